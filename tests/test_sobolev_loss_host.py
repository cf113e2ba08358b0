"""The Sobolev / L2 training losses without a GPU: the restatement of tests/sobolev_cases.py against the reference's own
float32 results (tests/golden/sobolev_loss_small.npz), its explicit adjoint against autograd, planted faults that the judged
rows must refuse, the ABI's refusals and the Python surface."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import judging
from tests import sobolev_cases as K

G = np.load(os.path.join(K.GOLDEN, "sobolev_loss_small.npz"))
GOLDEN_LIMIT = {torch.float64: 2e-6, torch.float32: 4e-6}      # the reference's float32 run against either restatement
GOLDEN_FORMS = [(f"{name}_{'rel' if rel else 'abs'}_{'fix' if fixed else 'per'}_{red}", 1 if name == "H1" else 0, rel, fixed, red)
                for name in ("H1", "Lp") for rel in (True, False) for fixed in ((False, True) if name == "H1" else (False,))
                for red in ("sum", "mean")]


@pytest.mark.parametrize("shape,d", K.GOLDEN_SHAPES, ids=[K.shape_id(s, d) for s, d in K.GOLDEN_SHAPES])
def test_restatement_against_the_reference(shape, d):
    """values and gradients of the reference's float32 run against the float64 and the float32 restatement, every form:
    d = 1, 2, 3, periodic and fixed, rel and abs, sum and mean, H1 and Lp; the stored inputs are the rebuilt ones"""
    x, y = K.make_inputs("white", shape, d)
    sid = K.shape_id(shape, d)
    assert np.array_equal(G[sid + "/x"], x.numpy()) and np.array_equal(G[sid + "/y"], y.numpy())
    h = K.uniform_h(shape, d)
    lines, bad = [], []
    for key, order, rel, fixed, red in GOLDEN_FORMS:
        for dtype in (torch.float64, torch.float32):
            r = K.restated(x, y, d, h, dtype, order=order, relative=rel, fix=(fixed,) * d, reductions=(red,))
            ev = judging.rel_err(torch.from_numpy(G[f"{sid}/{key}/value"]).reshape(r["value"].shape), r["value"])
            eg = judging.rel_err(torch.from_numpy(G[f"{sid}/{key}/grad"]), r["grad"])
            lines.append(f"{key:18s} {str(dtype)[6:]:8s} value {ev:10.3e}   grad {eg:10.3e}   limit {GOLDEN_LIMIT[dtype]:8.2e}")
            if not (ev < GOLDEN_LIMIT[dtype] and eg < GOLDEN_LIMIT[dtype]):
                bad.append(lines[-1])
    section = "host golden " + sid
    for line in lines:
        print(section, line)
    K.LOG.replace(section, lines)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("shape,d", [((2, 3, 2), 1), ((2, 2, 3), 1), ((2, 2, 5), 1), ((2, 2, 2, 3), 2), ((2, 2, 5, 4), 2),
                                     ((3, 2, 17, 33), 2), ((2, 1, 2, 3, 4), 3), ((2, 2, 5, 6, 7), 3)])
def test_adjoint_is_autograds(shape, d):
    """the explicit adjoint against autograd through the float64 restatement's forward: every boundary mode, rel and abs,
    H1 and Lp, a non-unit upstream gradient, extents down to 2 and 3"""
    x, y = K.make_inputs("white", shape, d)
    h = K.uniform_h(shape, d, tuple(1.0 + 0.5 * k for k in range(d)))
    g = [0.7 - 0.4 * c for c in range(shape[1])]
    for order, rel, fix in K.combos(d):
        kw = dict(order=order, relative=rel, fix=fix, reductions=("mean",), g=g)
        ref, auto = K.restated(x, y, d, h, torch.float64, **kw), K.autograd_reference(x, y, d, h, torch.float64, **kw)
        assert judging.rel_err(ref["grad"], auto["grad"]) < 1e-14, (order, rel, fix)
        assert judging.rel_err(ref["value"], auto["value"]) < 1e-15 and judging.rel_err(ref["planes"], auto["planes"]) < 1e-15


FAULT_CASE = dict(family="white", shape=(3, 2, 17, 33), d=2, fix=(True, False))


def test_float32_restatement_passes_its_own_rows():
    c = FAULT_CASE
    for family in K.FAMILIES:
        x, y, h, ref64, ref32 = K.references(family, c["shape"], c["d"], fix=c["fix"])
        assert not judging.rejected(K.loss_rows(ref32, ref64, ref32, c["d"]))


@pytest.mark.parametrize("fault", K.FAULTS)
def test_planted_fault_is_refused(fault):
    c = FAULT_CASE
    x, y, h, ref64, ref32 = K.references(c["family"], c["shape"], c["d"], fix=c["fix"])
    bad = K.restated(x, y, c["d"], h, torch.float32, fix=c["fix"], fault=fault)
    rows = K.loss_rows(bad, ref64, ref32, c["d"])
    refused = judging.rejected(rows)
    K.LOG.replace(f"host fault {fault}", [f"{n:22s} faulty {e:10.3e}   ref32 {r:10.3e}   floor {f:7.1e}" for n, e, r, f in rows]
                  + ["refused: " + ", ".join(refused)])
    assert refused, f"{fault}: every row passed"


def test_zero_difference_is_a_zero_gradient_in_the_restatement():
    x, y = K.make_inputs("white", (2, 2, 5), 1)
    r = K.restated(y, y, 1, [0.1], torch.float64)
    assert not bool(r["grad"].any()) and not bool(r["value"].any())


# ---------------------------------------------------------------------------------------------------------------------
# the ABI without a GPU
# ---------------------------------------------------------------------------------------------------------------------
EINVAL, EUNSUPPORTED = -1, -2
GOOD = dict(planes=6, channels=3, d=2, dims=(17, 33), order=1, relative=1, fix_mask=1, batch_reduce=1, ws_bytes=1 << 20)


def _abi_call(null=None, only=None, **change):
    """(forward rc, backward rc, forward message, backward message) of one refused call with fake pointers.  Every call made
    here is one that the checks stop: `only` = "forward" / "backward" leaves out the entry point that the change does not
    concern (None for its results), so nothing is ever launched on addresses that are no device memory."""
    assert null is not None or change, "the unchanged arguments would launch"
    from pde_policylearning_amd import _lib
    L = _lib.lib()
    a = dict(GOOD, **change)
    buf = (C.c_float * 4)()
    p = C.cast(buf, C.c_void_p)
    ptr = lambda name: None if name == null else p      # noqa: E731
    dims = None if a["dims"] is None else (C.c_int * 3)(*a["dims"])
    hh = (C.c_double * 3)(1.0, 1.0, 1.0)
    head = (a["planes"], a["channels"], a["d"], dims, a["order"], a["relative"], a["fix_mask"], a["batch_reduce"],
            None if null == "inv2h" else hh, None if null == "invh" else hh, 1.0, ptr("x"), ptr("y"))
    fwd = bwd = fmsg = bmsg = None
    if only in (None, "forward"):
        fwd = L.fno_sobolev_loss_forward(*head, ptr("value"), ptr("reduced"), ptr("ws"), a["ws_bytes"], None)
        fmsg = L.fno_last_error().decode()
    if only in (None, "backward"):
        bwd = L.fno_sobolev_loss_backward(*head, ptr("grad"), ptr("dx"), ptr("ws"), a["ws_bytes"], None)
        bmsg = L.fno_last_error().decode()
    return fwd, bwd, fmsg, bmsg


@pytest.mark.parametrize("change,code,word", [
    (dict(d=0), EINVAL, "d=0"), (dict(d=4), EINVAL, "d=4"), (dict(dims=(17, 1)), EINVAL, "extent 1"),
    (dict(dims=(0, 33)), EINVAL, "extent 0"), (dict(planes=0), EINVAL, "planes=0"), (dict(planes=-3), EINVAL, "planes=-3"),
    (dict(dims=None), EINVAL, "dims"), (dict(order=2), EINVAL, "order=2"), (dict(relative=2), EINVAL, "relative=2"),
    (dict(fix_mask=4), EINVAL, "fix_mask=4"), (dict(fix_mask=-1), EINVAL, "fix_mask=-1"),
    (dict(batch_reduce=3), EINVAL, "batch_reduce=3"), (dict(channels=4), EINVAL, "channels=4"),
    (dict(channels=0), EINVAL, "channels=0"), (dict(ws_bytes=16), EINVAL, "workspace too small"),
    (dict(dims=(65536, 32768)), EUNSUPPORTED, "2^31"), (dict(d=3, dims=(2048, 1024, 1024), fix_mask=0), EUNSUPPORTED, "2^31")])
def test_abi_refuses_before_launching(change, code, word):
    fwd, bwd, fmsg, bmsg = _abi_call(**change)
    assert (fwd, bwd) == (code, code), (fwd, bwd, fmsg, bmsg)
    assert word in fmsg and word in bmsg, (fmsg, bmsg)


@pytest.mark.parametrize("null", ["x", "y", "value", "reduced", "ws", "inv2h", "invh", "grad", "dx"])
def test_abi_refuses_null_pointers(null):
    if null in ("value", "reduced"):
        fwd, _, fmsg, _ = _abi_call(null=null, only="forward")
        assert fwd == EINVAL and "null" in fmsg
    elif null in ("grad", "dx"):
        _, bwd, _, bmsg = _abi_call(null=null, only="backward")
        assert bwd == EINVAL and "null" in bmsg
    else:
        fwd, bwd, fmsg, bmsg = _abi_call(null=null)
        assert (fwd, bwd) == (EINVAL, EINVAL) and "null" in fmsg and "null" in bmsg


def test_reduced_is_optional_without_a_batch_reduction():
    """...but the call still stops at the short workspace, before any launch"""
    fwd, _, fmsg, _ = _abi_call(null="reduced", only="forward", batch_reduce=0, ws_bytes=16)
    assert fwd == EINVAL and "workspace too small" in fmsg


def test_workspace_bytes_grow():
    from pde_policylearning_amd import _lib
    L = _lib.lib()
    nb = lambda planes, dims, order=1: L.fno_sobolev_loss_workspace_bytes(planes, len(dims), (C.c_int * 3)(*dims), order)      # noqa: E731
    base = nb(6, (61, 61))
    assert base >= 6 * 4 * 2 * 8 + 6 * 2 * 8            # 4 tiles a plane, two float64 sums a tile; (num, den) a plane
    assert nb(60, (61, 61)) > base and nb(6, (128, 128)) > base
    for dims in ((64,), (64, 64), (16, 64, 64)):
        sizes = [nb(p, tuple(4 * n for n in dims)) for p in (1, 64, 640)]
        assert sizes[0] > 0 and sizes == sorted(set(sizes)), sizes
    assert nb(640, (4096,), 0) > nb(640, (2048,), 0) > 0
    assert nb(0, (61, 61)) == 0 and nb(6, (61, 1)) == 0 and nb(6, (65536, 32768)) == 0 and nb(6, (61, 61), 2) == 0
    assert all(n in _lib.EXPORTED_SYMBOLS for n in ("fno_sobolev_loss_workspace_bytes", "fno_sobolev_loss_forward",
                                                    "fno_sobolev_loss_backward"))


def test_tile_extents_are_the_headers():
    src = open(os.path.join(K.ROOT, "pde_policylearning_amd", "csrc", "k_sobolev_loss.h")).read()
    const = lambda name: int(re.search(rf"constexpr int {name} = (\d+);", src).group(1))      # noqa: E731
    assert const("SOB_T0") == K.T0 and const("SOB_T1D_X") == K.T1
    assert (const("SOB_T2D_Y"), const("SOB_T2D_X")) == K.T2
    assert (const("SOB_T3D_Z"), const("SOB_T3D_Y"), const("SOB_T3D_X")) == K.T3
    assert "atomic" not in src.replace("no atomics", "")
    from pde_policylearning_amd import functional as F
    codes = {name: int(v) for name, v in re.findall(r"SOB_REDUCE_(\w+) = (\d+)", src)}
    assert F.SOBOLEV_REDUCE == {None: codes["NONE"], "sum": codes["SUM"], "mean": codes["MEAN"]}


# ---------------------------------------------------------------------------------------------------------------------
# the class surface
# ---------------------------------------------------------------------------------------------------------------------
def test_constructor_attributes():
    from pde_policylearning_amd.neuralop.training import H1Loss, LpLoss
    a = LpLoss()
    assert (a.d, a.p, a.reduce_dims, a.reductions, a.L) == (1, 2, [0], ["sum"], [2 * math.pi])
    b = LpLoss(d=2, L=1.0, reduce_dims=[0, 1], reductions=["sum", "mean"])
    assert (b.d, b.reduce_dims, b.reductions, b.L) == (2, [0, 1], ["sum", "mean"], [1.0, 1.0])
    c = LpLoss(d=3, reduce_dims=None, L=[1.0, 2.0, 3.0])
    assert c.reduce_dims is None and c.L == [1.0, 2.0, 3.0]
    h = H1Loss(d=2, fix_x_bnd=True, reductions="mean")
    assert (h.d, h.fix_x_bnd, h.fix_y_bnd, h.fix_z_bnd, h.reduce_dims, h.reductions) == (2, True, False, False, [0], ["mean"])
    assert h.L == [2 * math.pi] * 2
    with pytest.raises(AssertionError):
        H1Loss(d=4)
    with pytest.raises(AssertionError):
        LpLoss(reductions="max")
    for p in (1, 3):
        with pytest.raises(NotImplementedError, match=f"p={p}"):
            LpLoss(p=p)


def test_uniform_h_and_reduce_all():
    from pde_policylearning_amd.neuralop.training import H1Loss, LpLoss
    x = torch.zeros(2, 3, 5, 8)
    assert H1Loss(d=2, L=1.0).uniform_h(x) == [1.0 / 5, 1.0 / 8]
    assert LpLoss(d=1).uniform_h(x) == [2 * math.pi / 8]
    assert H1Loss(d=2, L=[3.0, 4.0]).uniform_h(x) == [3.0 / 5, 4.0 / 8]
    planes = torch.arange(6.0).reshape(2, 3)
    assert torch.equal(LpLoss(d=2).reduce_all(planes), planes.sum(0, keepdim=True))
    assert torch.equal(H1Loss(d=2, reduce_dims=[0, 1], reductions=["sum", "mean"]).reduce_all(planes),
                       planes.sum(0, keepdim=True).mean(1, keepdim=True))


def test_what_the_engine_has_no_kernel_for_says_so():
    from pde_policylearning_amd.neuralop.training import DissipativeLoss, H1Loss
    x = torch.zeros(2, 3, 8)
    with pytest.raises(NotImplementedError, match="compute_terms"):
        H1Loss().compute_terms(x, x, [0.1])
    with pytest.raises(NotImplementedError, match="DissipativeLoss"):
        DissipativeLoss(None, None, None, 1.0, (1.0, 2.0), 1, None)


def test_cpu_and_wrong_inputs_are_refused_by_name():
    from pde_policylearning_amd import functional as F
    from pde_policylearning_amd.neuralop.training import H1Loss, LpLoss
    x, y = torch.zeros(2, 3, 8, 8), torch.ones(2, 3, 8, 8)
    for call in (lambda: H1Loss(d=2)(x, y), lambda: H1Loss(d=2).abs(x, y), lambda: LpLoss(d=2)(x, y), lambda: LpLoss(d=2).abs(x, y),
                 lambda: H1Loss(d=2, reduce_dims=None)(x, y), lambda: F.sobolev_loss(x, y, 2, [0.1, 0.1])):
        with pytest.raises(RuntimeError, match="`x` must live on the GPU"):
            call()
    with pytest.raises(RuntimeError, match="`y` must be data"):
        H1Loss(d=2)(x, y.clone().requires_grad_(True))
    assert not F.sobolev_loss_supported(x, 2) and not F.sobolev_loss_supported(x.double(), 2)


def test_reference_import_line_resolves():
    """`from neuralop import LpLoss, H1Loss` (neuralop/__init__.py:9) with the package aliased as `neuralop`; what stays out of
    scope still says so"""
    import sys
    import pde_policylearning_amd.neuralop as pkg
    from pde_policylearning_amd.neuralop.training import losses
    names = ("neuralop", "neuralop.training", "neuralop.training.losses")
    saved = {k: sys.modules.get(k) for k in names}
    sys.modules["neuralop"], sys.modules["neuralop.training"], sys.modules["neuralop.training.losses"] = pkg, pkg.training, losses
    try:
        ns = {}
        exec("from neuralop import LpLoss, H1Loss", ns)
        exec("from neuralop.training.losses import LpLoss as L2, H1Loss as H2", ns)
        assert ns["LpLoss"] is losses.LpLoss and ns["H1Loss"] is losses.H1Loss and ns["L2"] is losses.LpLoss and ns["H2"] is losses.H1Loss
        for name in ("Trainer", "datasets", "mpu"):
            with pytest.raises(ImportError, match="out of scope"):
                exec(f"from neuralop import {name}", {})
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
