"""FNO blocks with the channel MLP (use_mlp=True) on the GPU: functional.channel_mlp (k_cmlp_fwd / k_cmlp_bwd, every
instantiation) and the models built on it, held to the float64 restatement of tests/channel_mlp_cases.py under the float32-budget
rule.  Every case asserts the kernel instantiation and its grid from the launch log before a number is compared; every measured
distance goes to profiles/r18_channel_mlp_errors.txt before anything is asserted."""
import numpy as np
import pytest
import torch

from tests import channel_mlp_cases as K
from tests.judging import dev  # noqa: F401

pytestmark = pytest.mark.gpu

CASES = {c["name"]: c for c in K.OP_CASES}
_REFS = {}


def _refs(case, scale, gate, gelu_out, x_grad=True):
    """(inputs, float32 reference, float64 reference) of a case, computed once and shared"""
    key = (case["name"], scale, gate, gelu_out, x_grad)
    if key not in _REFS:
        t = K.op_inputs(case, scale, gate)
        _REFS[key] = (t, K.op_reference(t, gelu_out, torch.float32, x_grad), K.op_reference(t, gelu_out, torch.float64, x_grad))
    return _REFS[key]


def _lds(C, H, backward):
    return ((C * (2 if backward else 1) + H) * 132 + H * (C + 1) + C * (H + 1) + H + 2 * C) * 4


def _check_launches(records, case, device, backward=True, gate=True):
    """the launch log of one forward (+ backward) of the op: instantiation, tiles, grid, block, LDS; returns the two grids"""
    C, H = case["C"], case["H"]
    ntiles = case["B"] * int(np.prod(case["dims"])) // 128
    ncu = torch.cuda.get_device_properties(device).multi_processor_count
    fwd = [r for r in records if r["name"] == "k_cmlp_fwd"]
    assert len(fwd) == 1, records
    per_cu = 2 if 2 * _lds(C, H, False) <= 160 * 1024 else 1
    want = dict(name="k_cmlp_fwd", variant=f"k_cmlp_fwd<{C}, {H}>", rb=0, ntiles=ntiles, grid=(min(ntiles, per_cu * ncu), 1, 1),
                block=(256, 1, 1), lds=_lds(C, H, False))
    assert fwd[0] == want, (fwd[0], want)
    if not backward:
        assert len(records) == 1, records
        return want["grid"][0], None
    bwd = [r for r in records if r["name"] == "k_cmlp_bwd"]
    red = [r for r in records if r["name"] == "k_reduce_jobs"]
    assert len(bwd) == 1 and len(red) == 1 and len(records) == 3, records
    wantb = dict(name="k_cmlp_bwd", variant=f"k_cmlp_bwd<{C}, {H}>", rb=0, ntiles=ntiles, grid=(min(ntiles, ncu), 1, 1),
                 block=(256, 1, 1), lds=_lds(C, H, True))
    assert bwd[0] == wantb, (bwd[0], wantb)
    assert red[0]["grid"] == (256, 5 if gate else 4, 1), red[0]
    return want["grid"][0], wantb["grid"][0]


def _run(case, dev, scale=1.0, gate=True, gelu_out=True, x_grad=True):  # noqa: F811
    from pde_policylearning_amd import _lib
    t, ref32, ref64 = _refs(case, scale, gate, gelu_out, x_grad)
    with _lib.launch_log() as log:
        got = K.op_engine(t, gelu_out, dev, x_grad)
        torch.cuda.synchronize()
    grids = _check_launches(log.records, case, dev, gate=gate)
    assert set(got) == set(ref64)
    return got, K.op_rows(got, ref32, ref64), grids


@pytest.mark.parametrize("gelu_out", [False, True])
@pytest.mark.parametrize("cname", list(CASES))
def test_op_against_float64(dev, cname, gelu_out):  # noqa: F811
    case = CASES[cname]
    got, rows, (gf, gb) = _run(case, dev, gelu_out=gelu_out)
    if cname == "896 tiles":          # the uneven persistent loop, in both kernels
        ntiles = case["B"] * 128
        assert ntiles > gf and ntiles % gf != 0 and ntiles > gb and ntiles % gb != 0, (ntiles, gf, gb)
    K.judge_budget(K.LOG, f"op {cname} C={case['C']} H={case['H']} B={case['B']} {case['dims']} gelu_out={int(gelu_out)}", rows)


@pytest.mark.parametrize("gelu_out", [False, True])
@pytest.mark.parametrize("cname", ["one tile", "width 32"])
def test_op_identity_skip(dev, cname, gelu_out):  # noqa: F811
    case = CASES[cname]
    got, rows, _ = _run(case, dev, gate=False, gelu_out=gelu_out)
    assert "dgate" not in got
    K.judge_budget(K.LOG, f"op {cname} identity skip gelu_out={int(gelu_out)}", rows)


@pytest.mark.parametrize("gelu_out", [False, True])
@pytest.mark.parametrize("scale", [1e-3, 1.0, 30.0])
def test_op_input_scales(dev, scale, gelu_out):  # noqa: F811
    """GELU's linear range, its knee and both saturated tails"""
    case = CASES["three tiles per sample"]
    _, rows, _ = _run(case, dev, scale=scale, gelu_out=gelu_out)
    K.judge_budget(K.LOG, f"op input scale {scale:g} gelu_out={int(gelu_out)}", rows)


def test_op_without_input_gradient(dev):  # noqa: F811
    """x needs no gradient: dx is not formed (the kernel gets a null pointer), everything else is what it was"""
    case = CASES["three tiles per sample"]
    got, rows, _ = _run(case, dev, x_grad=False)
    assert "dx" not in got
    full, _, _ = _run(case, dev)
    assert all(torch.equal(got[k], full[k]) for k in got)
    K.judge_budget(K.LOG, "op without dx", rows)


def test_op_is_the_same_in_both_gemm_modes(dev):  # noqa: F811
    """exact-fp32 MFMA in either mode: bitwise equal results"""
    from pde_policylearning_amd import _lib
    L = _lib.lib()
    case = CASES["3-D expansion 1"]
    old = L.fno_get_gemm_mode()
    res = {}
    try:
        for mode in (0, 1):
            L.fno_set_gemm_mode(mode)
            res[mode], rows, _ = _run(case, dev)
            K.judge_budget(K.LOG, f"op GEMM mode {mode}", rows)
    finally:
        L.fno_set_gemm_mode(old)
    assert all(torch.equal(res[0][k], res[1][k]) for k in res[0])


def test_op_is_repeatable_and_replays_in_a_graph(dev):  # noqa: F811
    """run twice and replayed from a captured graph: the same bits (no floating-point atomics, fixed-order reductions)"""
    from pde_policylearning_amd import functional as F
    case = CASES["three tiles per sample"]
    t, _, _ = _refs(case, 1.0, True, True)
    a = K.op_engine(t, True, dev)
    b = K.op_engine(t, True, dev)
    assert all(torch.equal(a[k], b[k]) for k in a)
    leaf = {k: v.to(dev).requires_grad_(True) for k, v in t.items() if k != "dy"}
    dy = t["dy"].to(dev)
    names = ("u", "x", "w1", "b1", "w2", "b2", "gate")

    def body():
        y = F.channel_mlp(*[leaf[k] for k in names], True)
        return y, torch.autograd.grad(y, [leaf[k] for k in names], dy)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):                      # one eager run loads the code objects before the capture
        body()
    torch.cuda.current_stream(dev).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y, grads = body()
    for _ in range(2):
        for g in (y,) + tuple(grads):
            g.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        got = dict(zip(("y", "du", "dx", "dw1", "db1", "dw2", "db2", "dgate"), (y,) + tuple(grads)))
        assert all(torch.equal(got[k], a[k]) for k in a)


@pytest.mark.parametrize("cname", list(K.MODEL_CASES))
def test_model_against_float64(dev, cname):  # noqa: F811
    """FNO2d / FNO3d with use_mlp=True: output and every parameter gradient against the float64 restatement; the distance to the
    reference's own stored float32 results is logged beside it (golden cases)"""
    from pde_policylearning_amd import _lib
    cls, pos, kw, shp, _ = K.MODEL_CASES[cname]
    p, x, g = K.model_params(cname)
    ref32, ref64 = K.model_reference(cname, p, x, torch.float32), K.model_reference(cname, p, x, torch.float64)
    with _lib.launch_log() as log:
        got, model = K.model_engine(cname, p, x, dev)
        torch.cuda.synchronize()
    C, L = pos[-1], kw["n_layers"]
    H = model.fno_blocks.mlp[0].hidden_channels
    ntiles = shp[0] * int(np.prod(shp[2:])) // 128
    fwd = [r for r in log.records if r["name"] == "k_cmlp_fwd"]
    bwd = [r for r in log.records if r["name"] == "k_cmlp_bwd"]
    assert len(fwd) == L and len(bwd) == L, log.records
    assert all(r["variant"] == f"k_cmlp_fwd<{C}, {H}>" and r["ntiles"] == ntiles and r["grid"][0] == ntiles for r in fwd), fwd
    assert all(r["variant"] == f"k_cmlp_bwd<{C}, {H}>" and r["ntiles"] == ntiles and r["grid"][0] == ntiles for r in bwd), bwd
    if len(shp) == 4:      # the Fourier part of every block ran as one fused engine layer (its skip's weight gradient included)
        assert sum(r["name"] == "k_block_bwd" for r in log.records) == L, [r["name"] for r in log.records]
    assert set(got) == set(ref64)
    rows = [(k, K.rel_err(got[k], r), K.rel_err(ref32[k], r), K.floor_of(k)) for k, r in ref64.items()]
    if g is not None:
        stored = {"y": g["y"], **{k: g["grads/" + k] for k in p}}
        for k, v in stored.items():
            print(f"model {cname} {k:46s} engine vs the reference's float32 {K.rel_err(got[k], torch.from_numpy(v).reshape(got[k].shape)):10.3e}")
    K.judge_budget(K.LOG, f"model {cname} {cls}{pos} {shp}", rows)
