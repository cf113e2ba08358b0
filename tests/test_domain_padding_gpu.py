"""Domain padding on the GPU (tests/domain_padding_cases.py): functional.domain_pad / domain_crop (k_domain_pad, k_domain_crop)
bitwise against torch.nn.functional.pad and slicing on the CPU, forward and backward, with the launch asserted from the launch
log; the neuralop models with domain_padding against the float64 restatement under the float32-budget rule, each with its
route asserted from the launch log.  Every measured distance goes to profiles/r22_domain_padding_errors.txt before anything is
asserted."""
import ctypes

import pytest
import torch

from tests import domain_padding_cases as K
from tests.judging import dev  # noqa: F401

pytestmark = pytest.mark.gpu

OPS = {c[0]: c for c in K.OP_CASES + [K.UNEVEN_CASE]}
_REFS = {}


def _ncu(device):
    return torch.cuda.get_device_properties(device).multi_processor_count


def _op_case(device, name, x=None, specials=True):
    """pad forward + backward and crop forward + backward of one case, each bitwise against the CPU and each one launch with
    the stated grid; returns the four launch records"""
    from pde_policylearning_amd import _lib
    from pde_policylearning_amd import functional as F
    _, shape, before, after = OPS[name]
    x = K.op_input(name, shape, specials) if x is None else x
    y_ref = K.pad(x, before, after)
    gy = K.op_input(name + ".gy", tuple(y_ref.shape), specials)         # the gradients travel as copies too
    recs = []

    def logged(fn, kernel, out_numel):
        with _lib.launch_log() as log:
            out = fn()
            torch.cuda.synchronize()
        want = K.expected_launch(kernel, out_numel, _ncu(device))
        assert log.records == [want], (log.records, want)
        recs.append(log.records[0])
        return out

    xd = x.to(device).requires_grad_(True)
    y = logged(lambda: F.domain_pad(xd, before, after), "k_domain_pad", y_ref.numel())
    assert y.shape == y_ref.shape and torch.equal(K.bits(y), K.bits(y_ref)), name
    gx, = logged(lambda: torch.autograd.grad(y, xd, gy.to(device)), "k_domain_crop", x.numel())
    assert torch.equal(K.bits(gx), K.bits(K.unpad(gy, before, after))), name
    yd = gy.to(device).requires_grad_(True)
    c = logged(lambda: F.domain_crop(yd, before, after), "k_domain_crop", x.numel())
    assert c.shape == x.shape and torch.equal(K.bits(c), K.bits(K.unpad(gy, before, after))), name
    gc, = logged(lambda: torch.autograd.grad(c, yd, xd.detach()), "k_domain_pad", y_ref.numel())
    assert torch.equal(K.bits(gc), K.bits(y_ref)), name
    # every margin element is +0.0: the whole image is compared above, and the margin of the reference is all-zero words
    margin = torch.ones(y_ref.shape, dtype=torch.bool)
    margin[(Ellipsis,) + tuple(slice(b, b + r) for b, r in zip(before, shape[2:]))] = False
    assert not bool(K.bits(y)[margin].any()) and not bool(K.bits(gc)[margin].any())
    return recs


@pytest.mark.parametrize("name", [c[0] for c in K.OP_CASES])
def test_op_is_a_bitwise_copy(dev, name):  # noqa: F811
    """NaN, both infinities and -0.0 sit in the interior (op_input) and arrive bit for bit; the margin is +0.0"""
    _op_case(dev, name)


def test_op_uneven_work_loop(dev):  # noqa: F811
    """more quads than the largest launch has threads, and no multiple of them: some threads make two trips, some one"""
    recs = _op_case(dev, K.UNEVEN_CASE[0], specials=False)
    for r in recs:
        threads = r["grid"][0] * r["block"][0]
        assert r["grid"][0] == K.GRID_PER_CU * _ncu(dev) and r["ntiles"] > threads and r["ntiles"] % threads != 0, r


def test_op_non_contiguous_and_misaligned_inputs(dev):  # noqa: F811
    """a non-contiguous operand is copied like the neighbours' (x.contiguous()); a contiguous view that starts 4, 8 or 12 bytes
    behind a 16-byte boundary takes the scalar loads on every row"""
    from pde_policylearning_amd import functional as F
    _, shape, before, after = OPS["2 nothing aligned"]
    x = K.op_input("noncontig", shape)
    want = K.pad(x, before, after)
    xt = x.to(dev).transpose(2, 3).contiguous().transpose(2, 3)
    assert not xt.is_contiguous()
    assert torch.equal(K.bits(F.domain_pad(xt, before, after)), K.bits(want))
    shape4 = (2, 3, 8, 12)
    x4 = K.op_input("misaligned", shape4)
    for off in (1, 2, 3):
        buf = torch.zeros(x4.numel() + 4, device=dev)
        view = buf[off:off + x4.numel()].view(shape4)
        view.copy_(x4.to(dev))
        assert view.is_contiguous() and view.data_ptr() % 16 == 4 * off
        assert torch.equal(K.bits(F.domain_pad(view, (0, 0), (0, 4))), K.bits(K.pad(x4, (0, 0), (0, 4))))
        y4 = K.pad(x4, (1, 4), (2, 4))
        buf = torch.zeros(y4.numel() + 4, device=dev)
        view = buf[off:off + y4.numel()].view(y4.shape)
        view.copy_(y4.to(dev))
        assert torch.equal(K.bits(F.domain_crop(view, (1, 4), (2, 4))), K.bits(x4))


@pytest.mark.parametrize("off", [1, 2, 3])
def test_abi_with_a_misaligned_output(dev, off):  # noqa: F811
    """the C ABI asks for 4-byte alignment only: with the output 4, 8 or 12 bytes behind a 16-byte boundary the elements in
    front of the first boundary and behind the last whole quad are written one by one, and nothing outside the tensor is"""
    from pde_policylearning_amd import _lib
    L = _lib.lib()
    _, shape, before, after = OPS["2 symmetric"]
    x = K.op_input("abi.misaligned", shape)
    y_ref = K.pad(x, before, after)
    ints = ctypes.c_int * 2
    args = (2, shape[0] * shape[1], ints(*shape[2:]), ints(*before), ints(*after))
    stream = torch.cuda.current_stream(dev).cuda_stream
    xd = x.to(dev)
    for fn, src, ref in ((L.fno_domain_pad, xd, y_ref), (L.fno_domain_crop, y_ref.to(dev), x)):
        buf = torch.full((ref.numel() + 8,), 7.0, device=dev)
        out = buf[off:off + ref.numel()]
        assert out.data_ptr() % 16 == 4 * off
        with _lib.launch_log() as log:
            _lib.check(fn(*args, src.data_ptr(), out.data_ptr(), stream), "domain pad / crop")
            torch.cuda.synchronize()
        assert len(log.records) == 1 and log.records[0]["ntiles"] == (ref.numel() - (4 - off)) // 4, log.records
        assert torch.equal(K.bits(out.view(ref.shape)), K.bits(ref))
        assert bool((buf[:off] == 7.0).all()) and bool((buf[off + ref.numel():] == 7.0).all())


def test_op_refuses_other_dtypes_and_shapes_before_any_launch(dev):  # noqa: F811
    """through the public wrappers, with real GPU tensors: float64 is refused naming float32, a tensor without a grid axis or
    with four of them by the shape rule, wrong amounts by name, a crop larger than the tensor; nothing is launched"""
    from pde_policylearning_amd import _lib
    from pde_policylearning_amd import functional as F
    with _lib.launch_log() as log:
        for fn in (F.domain_pad, F.domain_crop):
            with pytest.raises(RuntimeError, match="float32"):
                fn(torch.zeros(2, 3, 8, 8, dtype=torch.float64, device=dev), (0, 0), (1, 1))
            with pytest.raises(RuntimeError, match=r"d1\[, d2\[, d3\]\]"):
                fn(torch.zeros(2, 3, device=dev), (), ())
            with pytest.raises(RuntimeError, match=r"d1\[, d2\[, d3\]\]"):
                fn(torch.zeros(1, 1, 2, 2, 2, 2, device=dev), 0, 1)
            with pytest.raises(RuntimeError, match="non-negative"):
                fn(torch.zeros(2, 3, 8, 8, device=dev), (0, 0), (1, -1))
            with pytest.raises(RuntimeError, match="non-negative"):
                fn(torch.zeros(2, 3, 8, 8, device=dev), (0,), (1, 1))
        with pytest.raises(RuntimeError, match="larger than its pads"):
            F.domain_crop(torch.zeros(2, 3, 4, 8, device=dev), (2, 0), (2, 0))
    assert log.records == []


def test_op_replays_in_a_graph(dev):  # noqa: F811
    """no host synchronisation, nothing allocated by the library: pad and crop are captured and replayed"""
    from pde_policylearning_amd import functional as F
    _, shape, before, after = OPS["6 3-D symmetric"]
    x = K.op_input("graph", shape).to(dev)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):                      # one eager run loads the code objects before the capture
        F.domain_crop(F.domain_pad(x, before, after), before, after)
    torch.cuda.current_stream(dev).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y = F.domain_pad(x, before, after)
        z = F.domain_crop(y, before, after)
    for _ in range(2):
        y.fill_(float("nan"))
        z.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(K.bits(y), K.bits(K.pad(x.cpu(), before, after))) and torch.equal(K.bits(z), K.bits(x))


# ---------------------------------------------------------------------------------------------------------------------
# models
# ---------------------------------------------------------------------------------------------------------------------
def _refs(cname):
    """(parameters, input, float32 reference, float64 reference) of a model case, computed once and shared"""
    if cname not in _REFS:
        p, x = K.model_params(cname)
        _REFS[cname] = (p, x, K.model_reference(cname, p, x, torch.float32), K.model_reference(cname, p, x, torch.float64))
    return _REFS[cname]


def _no_torch_pad(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("torch.nn.functional.pad was called on the engine route")
    monkeypatch.setattr(torch.nn.functional, "pad", refuse)


def _run_model(cname, device, monkeypatch, fused, label=None):
    """one forward + backward of a model case: the route from the launch log, then every distance under the budget rule.
    fused: the blocks ran as ONE fused engine stack (a block backward kernel per layer, no standalone spectral convolution);
    False: the per-layer composition (no block kernel at all); None: not stated for the case"""
    from pde_policylearning_amd import _lib
    p, x, ref32, ref64 = _refs(cname)
    with monkeypatch.context() as mp:
        _no_torch_pad(mp)
        with _lib.launch_log() as log:
            got, model = K.model_engine(cname, p, x, device)
            torch.cuda.synchronize()
    names = [r["name"] for r in log.records]
    padded = K.MODEL_CASES[cname][4]
    assert model.domain_padding.padded_resolution(x.shape[2:]) == padded
    # the pad kernel once per forward and once more in the backward (the crop's adjoint); the crop kernel likewise
    assert names.count("k_domain_pad") == 2 and names.count("k_domain_crop") == 2, names
    first = {k: names.index(k) for k in ("k_domain_pad", "k_domain_crop")}
    assert first["k_domain_pad"] < first["k_domain_crop"], names
    ncu = _ncu(device)
    hidden = model.hidden_channels
    n_in, n_pad = x.shape[0] * hidden * int(torch.Size(x.shape[2:]).numel()), x.shape[0] * hidden * int(torch.Size(padded).numel())
    assert [r for r in log.records if r["name"] == "k_domain_pad"] == [K.expected_launch("k_domain_pad", n_pad, ncu)] * 2
    assert [r for r in log.records if r["name"] == "k_domain_crop"] == [K.expected_launch("k_domain_crop", n_in, ncu)] * 2
    nblock = sum(n.startswith("k_block_bwd") for n in names)
    if fused is True:
        assert nblock == K.N_LAYERS, names
    elif fused is False:
        assert nblock == 0, names
    assert set(got) == set(ref64)
    K.judge_budget(K.LOG, f"model {label or cname} {K.MODEL_CASES[cname][0]}{K.MODEL_CASES[cname][1]} {tuple(x.shape)} -> {padded}",
                   K.model_rows(got, ref32, ref64))
    return names, got


@pytest.mark.parametrize("mode", [1, 0])
def test_model_tiled(dev, monkeypatch, mode):  # noqa: F811
    """48 x 48 at 1/3 -> 64 x 64: whole rows, one fused stack in either GEMM mode"""
    from pde_policylearning_amd import _lib
    L = _lib.lib()
    old = L.fno_get_gemm_mode()
    try:
        L.fno_set_gemm_mode(mode)
        _run_model("tiled", dev, monkeypatch, fused=True, label=f"tiled GEMM mode {mode}")
    finally:
        L.fno_set_gemm_mode(old)


def test_model_tiled_symmetric(dev, monkeypatch):  # noqa: F811
    """32 x 32 at 0.5 on both sides -> 64 x 64"""
    _run_model("tiled symmetric", dev, monkeypatch, fused=True)


@pytest.mark.parametrize("mode", [1, 0])
def test_model_loose(dev, monkeypatch, mode):  # noqa: F811
    """64 x 64 at 0.25 -> 80 x 80: loose rows, the fused stack in split precision; in exact-fp32 mode the block kernels do not
    cover loose rows and the model takes the per-layer composition"""
    from pde_policylearning_amd import _lib
    L = _lib.lib()
    old = L.fno_get_gemm_mode()
    try:
        L.fno_set_gemm_mode(mode)
        _run_model("loose", dev, monkeypatch, fused=mode == 1, label=f"loose GEMM mode {mode}")
    finally:
        L.fno_set_gemm_mode(old)


def test_model_unfused(dev, monkeypatch):  # noqa: F811
    """32 x 32 at 0.25 -> 40 x 40: 1600 pixels are no multiple of 128, so every layer is a standalone spectral convolution and
    a torch skip"""
    names, _ = _run_model("unfused", dev, monkeypatch, fused=False)
    assert any(n.startswith(("k_lift", "k_proj")) for n in names), names       # lifting and projection at 32 x 32 stay on the engine


def test_model_non_square(dev, monkeypatch):  # noqa: F811
    """32 x 64 at 0.25 -> 40 x 80 (each axis by its own amount; the reference would return (40, 56)): the output has the input's
    grid"""
    _, got = _run_model("non-square", dev, monkeypatch, fused=True)
    assert tuple(got["y"].shape) == (2, 1, 32, 64)


def test_model_mlp(dev, monkeypatch):  # noqa: F811
    """use_mlp=True at width 64 on 48 x 48 -> 64 x 64: the layer loop on the padded tensor, one channel-MLP kernel per layer
    and direction on the padded grid"""
    names, _ = _run_model("mlp", dev, monkeypatch, fused=None)
    assert names.count("k_cmlp_fwd") == K.N_LAYERS and names.count("k_cmlp_bwd") == K.N_LAYERS, names
    assert sum(n.startswith("k_block_bwd") for n in names) == K.N_LAYERS, names      # each Fourier part: one fused engine layer


def test_model_3d(dev, monkeypatch):  # noqa: F811
    """FNO3d on 16^3 at 1.0 -> 32^3"""
    _run_model("3-D", dev, monkeypatch, fused=True)


def test_model_1d(dev, monkeypatch):  # noqa: F811
    """FNO1d on N = 256 at 0.5 -> 384: the 1-D kernels run on the padded length"""
    names, _ = _run_model("1-D", dev, monkeypatch, fused=None)
    assert any(n.startswith("k_s1_") for n in names), names


def test_fno1d_shape_rule_applies_to_the_padded_length(dev):  # noqa: F811
    from pde_policylearning_amd import _lib
    from pde_policylearning_amd.neuralop.models import FNO1d
    model = FNO1d(16, 32, domain_padding=0.25).to(dev)
    with _lib.launch_log() as log:
        with pytest.raises(RuntimeError, match=r"padded to N = 320.*multiple of 128"):
            model(torch.zeros(2, 3, 256, device=dev))
    assert log.records == []


def test_direct_write_bucket_does_not_accumulate(dev):  # noqa: F811
    """FlatGradBucket(direct_module=model) never clears a direct module's gradients; the padded route hands every gradient to
    autograd, which accumulates, so forward() clears them: two passes on one batch leave the first pass's gradients, bitwise"""
    from pde_policylearning_amd.trainer import FlatGradBucket
    p, x, _, _ = _refs("tiled")
    model = K.load_model("tiled", p, dev)
    bucket = FlatGradBucket(model.parameters(), direct_module=model)
    xd = x.to(dev)
    grads = []
    for _ in range(2):
        bucket.zero()
        model(xd).square().sum().backward()
        grads.append({n: q.grad.detach().clone() for n, q in model.named_parameters()})
    assert all(float(g.abs().max()) > 0 for g in grads[0].values())
    assert all(torch.equal(K.bits(grads[0][n]), K.bits(grads[1][n])) for n in grads[0]), [n for n in grads[0] if not torch.equal(grads[0][n], grads[1][n])]


def test_domain_padding_zero_is_the_unpadded_model(dev):  # noqa: F811
    """domain_padding=0 on the tiled grid: the whole-model fused plan, launch for launch and bit for bit what a model built
    without the argument gives"""
    from pde_policylearning_amd import _lib
    p, _, _, _ = _refs("tiled")
    x = torch.from_numpy(K.fill_named("input:dompad.zero.x", (2, 3, 64, 64), 1.0)).to(dev)
    outs, logs = [], []
    for override in (dict(domain_padding=0), dict(domain_padding=None)):
        model = K.load_model("tiled", p, dev, **override)
        assert model.domain_padding is None and model.fused_supported(x)
        with _lib.launch_log() as log:
            y = model(x)
            y.square().sum().backward()
            torch.cuda.synchronize()
        outs.append({"y": y.detach(), **{n: q.grad for n, q in model.named_parameters()}})
        logs.append(log.records)
    assert logs[0] == logs[1] and logs[0]
    names = [r["name"] for r in logs[0]]
    assert not [n for n in names if n.startswith("k_domain")]
    # the whole-model plan: block 0's backward takes the model input and forms the lifting's gradients itself (k_block_bwd0,
    # launched only by a plan with a lifting), one block backward per layer in all, and neither the standalone lifting nor the
    # standalone spectral convolution of the layer routes
    assert names.count("k_block_bwd0") == 1 and sum(n.startswith("k_block_bwd") for n in names) == K.N_LAYERS, names
    assert "k_lift_bwd" not in names and "k_lift_dx" not in names, names
    assert all(torch.equal(K.bits(outs[0][k]), K.bits(outs[1][k])) for k in outs[0])
