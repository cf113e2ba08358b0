"""The standalone spectral convolution on the GPU against oracle/fno_oracle.py in float64, one case per dispatch route and
edge of fno_spec_forward / fno_spec_backward (fno_abi.hip: row_forward, row_inverse, axis_pass, mode_gemm, mode_gemm_dw).
Cases, references, sliced quantities and the criterion: tests/spec_conv_cases.py (shown to bite, and to be passable, on the CPU
in tests/test_spec_conv_reference.py).

Which kernel a shape reaches depends on the tile count against the device's compute units, so the FIRST assertion of every case
reads the library's launch log (fno_debug_launch_log: recorded by the launching statement) and requires the variant, the rows
per workgroup, a persistent grid smaller than its tile count and the partial last block the case was chosen for - on a device
with another CU count the case fails naming the route it took instead of passing on another one.  The expectations below are
for 256 compute units.  Every launch goes to the file $SPEC_CONV_ROUTE_LOG names (profiles/r14_spec_conv_routes.txt), every
judged quantity to $SPEC_CONV_ERROR_LOG (profiles/r14_spec_conv_errors.txt)."""
import os

import pytest
import torch

from tests import spec_conv_cases as C
from tests.judging import dev  # noqa: F401

pytestmark = pytest.mark.gpu
ROUTE_LOG_ENV = "SPEC_CONV_ROUTE_LOG"


# variant -> what every launch of it in the case must show.  rb / ntiles / grid (x extent) / block (x extent): equal;
# loops: ntiles > workgroups (a persistent loop with uneven shares); partial: P % rb != 0; even: P % rb == 0
ROUTES = {
    "rows rb2 partial": {"k_rowdft_chan<16,16>": dict(rb=2, partial=True), "k_rowidft_chan<16>": dict(rb=2, partial=True)},
    "rows rb4 partial loop": {"k_rowdft_chan<16,16>": dict(rb=4, partial=True, ntiles=1058, grid=1024, loops=True),
                              "k_rowidft_chan<16>": dict(rb=4, partial=True, ntiles=1058)},
    "rows mfma rb4 partial": {"k_rowidft_chan_mfma<16>": dict(rb=4, partial=True, ntiles=1058),
                              "k_rowdft_chan<16,16>": dict(rb=4, partial=True, loops=True)},
    "rows rb1 loop 32": {"k_rowdft_chan<16,16>": dict(rb=1, ntiles=1055, grid=1024, loops=True), "k_rowidft_chan_mfma<16>": dict(rb=1)},
    "rows rb1 loop 34": {"k_rowdft_chan<16,16>": dict(rb=1, ntiles=1055, grid=1024, loops=True), "k_rowidft_chan<16>": dict(rb=1)},
    "chan4 q4 loop": {"k_rowdft_chan4<16>": dict(rb=4, ntiles=1536, grid=1024, loops=True)},
    "chan4 rb16 loop": {"k_rowdft_chan4<16>": dict(rb=16, ntiles=1152, grid=1024, loops=True)},
    "flat tile partial": {"k_rowdft_chan4<16>": dict(), "k_rowidft_flat_mfma<16>": dict(grid=(24 * 43 * 41 + 255) // 256)},
    "tile loop uneven": {"k_rowdft_tile<32,128>": dict(ntiles=784, grid=768, loops=True),
                         "k_pw_fwd<2,32,128>": dict(ntiles=784, grid=512, loops=True)},
    "gelu chan4": {"k_rowdft_chan4<16>(act_in)": dict()},
    "gemm lds 48>64": {"k_mode_gemm_lds<2>": dict(rb=16), "k_mode_gemm_dw_lds<2>": dict(rb=16)},
    "gemm lds 40>64": {"k_mode_gemm_lds<2>": dict(rb=16), "k_mode_gemm_dw_lds<2>": dict(rb=16)},
    "gemm lds 128>128": {"k_mode_gemm_lds<2>": dict(rb=8), "k_mode_gemm_dw_lds<2>": dict(rb=8)},
    "gemm plain 34>20": {"k_mode_gemm": dict(), "k_mode_gemm_dw": dict(rb=12)},
    "gemm plain 64>96": {"k_mode_gemm": dict(rb=2), "k_mode_gemm_dw": dict(rb=2)},
    "axis 3d dead planes": {"k_axis_fwd<4>": dict(), "k_axis_fwd<6>": dict(), "k_axis_inv<4>": dict(), "k_axis_inv<6>": dict()},
    "axis sweep 320": {"k_axis_generic(truncating)": dict(), "k_axis_generic(extending)": dict()},
    "overlap A": {"k_axis_fwd<12>": dict(), "k_axis_inv<12>": dict()},
    "dbias scalar arm": {"k_channel_sums": dict()},
}
for _b in (2, 3, 4):
    ROUTES[f"stream B{_b}"] = {f"k_mode_gemv<{_b}>": dict(grid=(714 + 3) // 4), f"k_mode_outer_dw<{_b}>": dict(grid=(714 + 3) // 4),
                               "k_axis_generic(truncating)": dict(), "k_axis_generic(extending)": dict()}
for _i, _m in enumerate(C.AXIS_M):
    _t = ",tlds" if 2 * _m >= 24 else ""
    ROUTES[f"axis m{_m} {'B' if _i % 2 else 'C'}"] = (
        {"k_axis_generic(truncating)": dict(), "k_axis_generic(extending)": dict()} if _m == 7 else
        {f"k_axis_fwd<{2 * _m}{_t}>": dict(), f"k_axis_inv<{2 * _m}{_t}>": dict()})
assert set(ROUTES) == set(C.CASE)


def _fmt(r):
    return (f"{r['name']:<18s} {r['variant'] or '-':<34s} rb {r['rb']:3d}  ntiles {r['ntiles']:6d}  grid {str(r['grid']):<18s} "
            f"block {str(r['block']):<14s} lds {r['lds']:6d}")


def route_failures(case, records):
    """what the launch log of one case lacks, as a list of messages (each names the routes that were taken)"""
    path = os.environ.get(ROUTE_LOG_ENV)
    if path:
        with open(path, "a") as f:
            f.write(f"# {case.name}: {case.dialect} B={case.B} {case.cin}->{case.cout} dims={case.dims} modes={case.modes}"
                    f"{' input_gelu' if case.gelu else ''}  P={case.P} Ktot={case.Ktot}\n")
            f.writelines("  " + _fmt(r) + "\n" for r in records)
    took = "\n".join(_fmt(r) for r in records)
    bad = []
    for variant, want in ROUTES[case.name].items():
        recs = [r for r in records if (r["variant"] or r["name"]) == variant]
        if not recs:
            bad.append(f"{case.name}: no launch of {variant}")
        for r in recs:
            wgs = r["grid"][0] * r["grid"][1] * r["grid"][2]
            checks = {"rb": lambda v: r["rb"] == v, "ntiles": lambda v: r["ntiles"] == v, "grid": lambda v: r["grid"][0] == v,
                      "block": lambda v: r["block"][0] == v, "loops": lambda v: (r["ntiles"] > wgs) == v,
                      "partial": lambda v: r["rb"] > 1 and (case.P % r["rb"] != 0) == v}
            bad += [f"{case.name}: {variant} is not at {k} = {v}: {_fmt(r)}" for k, v in want.items() if not checks[k](v)]
    return [b + "\nthe case took\n" + took for b in bad]


def engine_eval(case, inp, dev, grads=("x", "w", "bias"), bias=None):
    """({"y", "dx", "dw" (oracle corner order, complex), "dbias"} on the CPU, the launch records) of forward + backward;
    grads: the operands that require a gradient (the others reach fno_spec_backward as NULL); bias: one to use in a dialect
    that has none"""
    from pde_policylearning_amd import _lib
    from pde_policylearning_amd import functional as F
    order = C.engine_order(case)
    x = inp["x"].to(dev).requires_grad_("x" in grads)
    ws = [w.to(dev).requires_grad_("w" in grads) for w in inp["w"]]
    bias = inp["bias"] if bias is None else bias
    be = bias.to(dev).requires_grad_("bias" in grads) if bias is not None else None
    with _lib.launch_log() as log:
        if case.gelu:        # the spectral branch alone: pointwise weight zero, no bias
            y = F.spectral_pointwise_layer(x, [ws[i] for i in order], case.live, C.NORM[case.dialect],
                                           torch.zeros(case.cin, case.cin, 1, device=dev), None, input_gelu=True,
                                           weight_last_extent=case.modes[-1])
        else:
            y = F.spectral_conv(x, [ws[i] for i in order], be, case.live, C.NORM[case.dialect], weight_last_extent=case.modes[-1])
        y.backward(inp["dy"].to(dev))
        torch.cuda.synchronize()
    out = {"y": y.detach().cpu(), "dx": x.grad.cpu() if x.grad is not None else None,
           "dw": [torch.view_as_complex(w.grad.cpu()) for w in ws] if ws[0].grad is not None else None,
           "dbias": be.grad.reshape(-1).cpu() if be is not None and be.grad is not None else None}
    return out, log.records


def _run(case, dev):
    inp, ref64, ref32 = C.references(case.name)
    got, records = engine_eval(case, inp, dev)
    bad = route_failures(case, records)
    assert not bad, "\n".join(bad)
    assert all(bool(torch.isfinite(t).all()) for t in [got["y"], got["dx"]] + got["dw"])
    bad = C.failures(case, got, ref32, ref64, inp)
    assert not bad, "\n".join(bad)
    return got, records


@pytest.mark.parametrize("name", [c.name for c in C.ROW_CASES], ids=[c.id for c in C.ROW_CASES])
def test_row_pass_routes_vs_float64(dev, name):
    _run(C.CASE[name], dev)


@pytest.mark.parametrize("name", [c.name for c in C.STREAM_CASES + C.GEMM_CASES], ids=[c.id for c in C.STREAM_CASES + C.GEMM_CASES])
def test_contraction_routes_vs_float64(dev, name):
    case = C.CASE[name]
    _, records = _run(case, dev)
    if case in C.GEMM_CASES:        # the edges: a last batch chunk and (40 -> 64) a last input-channel chunk that are not full
        fwd = [r for r in records if r["name"] == "k_mode_gemm"][0]
        dw = [r for r in records if r["name"] == "k_mode_gemm_dw"][0]
        assert case.B % fwd["rb"] != 0 and fwd["grid"][:2] == (case.Ktot, -(-case.B // fwd["rb"])), fwd
        assert dw["grid"][:2] == (case.Ktot, -(-case.cin // dw["rb"])) and (case.cin % dw["rb"] != 0) == (case.cin in (40, 34)), dw
    else:
        assert case.Ktot == 714 and case.Ktot % 4 == 2


@pytest.mark.parametrize("name", [c.name for c in C.AXIS_CASES + C.DBIAS_CASES], ids=[c.id for c in C.AXIS_CASES + C.DBIAS_CASES])
def test_leading_axis_and_bias_routes_vs_float64(dev, name):
    case = C.CASE[name]
    _, records = _run(case, dev)
    if case in C.DBIAS_CASES:
        assert (case.P * case.dims[-1]) % 4 != 0
    if name.startswith("axis m"):
        assert (case.live[-1] * case.cin) % 64 != 0


NULL_ARM_CASES = C.MULTI_ROW + C.STREAM_CASES[:1]


@pytest.mark.parametrize("name", [c.name for c in NULL_ARM_CASES], ids=[c.id for c in NULL_ARM_CASES])
def test_null_arms_leave_the_other_gradients_bit_identical(dev, name):
    """dx, dW and dbias each left out in turn (the NULL arms of fno_spec_backward; the cases are dialect C, so a bias is added for
    the purpose): what is still requested equals the full call bit for bit, and the route is the full call's minus what only the
    omitted gradient needs"""
    case = C.CASE[name]
    inp = C.references(name)[0]
    from oracle.detfill import fill_named
    bias = torch.from_numpy(fill_named("sc.null.bias", (case.cout,), 0.1))
    full, records = engine_eval(case, inp, dev, bias=bias)
    bad = route_failures(case, records)
    assert not bad, "\n".join(bad)
    assert full["dbias"] is not None
    for left_out in ("x", "w", "bias"):
        part, recs = engine_eval(case, inp, dev, grads=tuple(g for g in ("x", "w", "bias") if g != left_out), bias=bias)
        names = [r["name"] for r in recs]
        assert ("k_channel_sums" in names) == (left_out != "bias") and ("k_unpack_dw" in names) == (left_out != "w"), names
        assert len([n for n in names if n.startswith("k_rowidft")]) == (1 if left_out == "x" else 2), names
        assert torch.equal(part["y"], full["y"])
        for k, key in (("x", "dx"), ("bias", "dbias")):
            assert (part[key] is None) if k == left_out else torch.equal(part[key], full[key]), (left_out, key)
        if left_out == "w":
            assert part["dw"] is None
        else:
            assert all(torch.equal(torch.view_as_real(a), torch.view_as_real(b)) for a, b in zip(part["dw"], full["dw"])), left_out
