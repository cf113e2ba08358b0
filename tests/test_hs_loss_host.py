"""The spectral Sobolev loss without a GPU: the restatement of tests/hs_loss_cases.py against the reference's own float32
results (tests/golden/hs_loss_small.npz), its explicit adjoint against autograd, its single-mode closed form, planted faults
that the judged rows must refuse, the ABI's refusals and the Python surface."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from tests import hs_loss_cases as K
from tests import judging

G = np.load(os.path.join(K.GOLDEN, "hs_loss_small.npz"))
# the reference's float32 run against either restatement: the rule of tests/test_sobolev_loss_host.py for its golden file
GOLDEN_LIMIT = {torch.float64: 2e-6, torch.float32: 4e-6}


def test_restatement_against_the_reference():
    """losses (mean, sum, per sample) and gradients (mean; the stored even rows) of the reference's float32 run against the
    float64 and the float32 restatement, every form; the inputs are rebuilt from the stored names' scales.  The file is data
    only and small."""
    assert os.path.getsize(os.path.join(K.GOLDEN, "hs_loss_small.npz")) < 100 * 1024
    assert tuple(G["shape"]) == K.GOLDEN_SHAPE and {n: float(G[f"scale/{n}"]) for n in ("x", "y")} == K.GOLDEN_SCALES
    x, y = K.golden_inputs()
    lines, bad = [], []
    for k, a, group in K.FORMS:
        for red in K.REDUCTIONS:
            key = f"{K.form_id(k, a, group)}/{red}"
            for dtype in (torch.float64, torch.float32):
                r = K.restated(x, y, dtype, k, a, group, red)
                ev = judging.rel_err(torch.from_numpy(G[key + "/value"]).reshape(r["value"].shape), r["value"])
                eg = judging.rel_err(torch.from_numpy(G[key + "/grad_even_rows"]), r["grad"][:, ::2]) if red == "mean" else 0.0
                lines.append(f"{key:34s} {str(dtype)[6:]:8s} value {ev:10.3e}   grad {eg:10.3e}   limit {GOLDEN_LIMIT[dtype]:8.2e}")
                if not (ev < GOLDEN_LIMIT[dtype] and eg < GOLDEN_LIMIT[dtype]):
                    bad.append(lines[-1])
    section = "host golden " + K.shape_id(K.GOLDEN_SHAPE)
    for line in lines:
        print(section, line)
    K.LOG.replace(section, lines)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("shape", [(2, 32, 32, 3), (2, 32, 32, 2, 2), (3, 32, 32)], ids=K.shape_id)
def test_adjoint_is_autograds(shape):
    """the explicit adjoint against autograd through the composition of torch operations, float64: every form and reduction with
    its upstream gradient"""
    x, y = K.make_inputs("white", shape)
    for k, a, group in K.FORMS:
        for red in K.REDUCTIONS:
            g = K.upstream(red, shape[0])
            ref, auto = K.restated(x, y, torch.float64, k, a, group, red, g), K.autograd_reference(x, y, torch.float64, k, a, group, red, g)
            assert judging.rel_err(ref["grad"], auto["grad"].reshape(shape)) < 1e-12, (k, a, group, red)
            assert judging.rel_err(ref["value"], auto["value"]) < 1e-13 and judging.rel_err(ref["samples"], auto["samples"]) < 1e-13


@pytest.mark.parametrize("n", [32, 128])
def test_single_modes_in_the_restatement(n):
    """the closed form of tests/test_hs_loss_gpu.py::test_single_modes against the float64 restatement on exact (float64) modes"""
    pairs = K.mode_pairs(n)
    for k, a in ((2, (0.5, 0.25)), (1, None)):
        for i, pe in enumerate(pairs):
            py = pairs[(i + 1) % len(pairs)]
            y = torch.from_numpy(K.cosine_mode(n, *py, 1.0)).reshape(1, n, n)
            x = y + torch.from_numpy(K.cosine_mode(n, *pe, 0.5)).reshape(1, n, n)
            got, want = float(K.restated(x, y, torch.float64, k, a)["value"]), K.mode_loss(n, pe, 0.5, py, 1.0, k, a)
            assert abs(got - want) < 1e-9 * want, (n, k, pe, py, got, want)


FAULT_CASE = dict(family="white", shape=(2, 32, 32, 3), k=2, a=(0.5, 0.25))


def test_float32_restatement_passes_its_own_rows():
    c = FAULT_CASE
    for family in K.FAMILIES:
        for group in (False, True):
            x, y, ref64, ref32 = K.references(family, c["shape"], c["k"], c["a"], group)
            assert not judging.rejected(K.loss_rows({"value": ref32["value"], "grad": ref32["grad"]}, ref64, ref32))


@pytest.mark.parametrize("fault", K.FAULTS)
def test_planted_fault_is_refused(fault):
    c = FAULT_CASE
    k, group = (3, True) if fault == "divisor_terms" else (c["k"], False)
    x, y, ref64, ref32 = K.references(c["family"], c["shape"], k, c["a"][:min(k, 2)] + (1.0,) * (k - 2), group)
    bad = K.restated(x, y, torch.float32, k, c["a"][:min(k, 2)] + (1.0,) * (k - 2), group, fault=fault)
    rows = K.loss_rows({"value": bad["value"], "grad": bad["grad"]}, ref64, ref32)
    refused = judging.rejected(rows)
    K.LOG.replace(f"host fault {fault}", [f"{n:22s} faulty {e:10.3e}   ref32 {r:10.3e}   floor {f:7.1e}" for n, e, r, f in rows]
                  + ["refused: " + ", ".join(refused)])
    assert refused, f"{fault}: every row passed"


def test_zero_difference_is_a_zero_gradient_in_the_restatement():
    _, y = K.make_inputs("white", (2, 32, 32, 3))
    for group in (False, True):
        r = K.restated(y, y, torch.float64, 2, (0.5, 0.25), group)
        assert not bool(r["grad"].any()) and not bool(r["value"].any())


# ---------------------------------------------------------------------------------------------------------------------
# the ABI without a GPU
# ---------------------------------------------------------------------------------------------------------------------
EINVAL = -1
GOOD = dict(batch=2, nx=32, ny=32, channels=3, terms=2, w2=(1.0, 1.0, 0.0), group=0, divisor=2.0, reduce=2, ws_bytes=1 << 16)


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
    w2 = None if null == "w2" else (C.c_double * 3)(*a["w2"])
    head = (a["batch"], a["nx"], a["ny"], a["channels"], a["terms"], w2, a["group"], a["divisor"], a["reduce"], ptr("x"), ptr("y"))
    fwd = bwd = fmsg = bmsg = None
    if only in (None, "forward"):
        fwd = L.fno_hs_loss_forward(*head, ptr("value"), ptr("reduced"), ptr("ws"), a["ws_bytes"], None)
        fmsg = L.fno_last_error().decode()
    if only in (None, "backward"):
        bwd = L.fno_hs_loss_backward(*head, ptr("grad"), ptr("dx"), ptr("ws"), a["ws_bytes"], None)
        bmsg = L.fno_last_error().decode()
    return fwd, bwd, fmsg, bmsg


@pytest.mark.parametrize("change,word", [
    (dict(nx=48, ny=48), "48 x 48"), (dict(nx=32, ny=64), "32 x 64"), (dict(nx=256, ny=256), "256 x 256"), (dict(nx=0, ny=0), "0 x 0"),
    (dict(batch=0), "batch=0"), (dict(batch=-2), "batch=-2"), (dict(channels=0), "channels=0"), (dict(terms=4), "terms=4"),
    (dict(terms=0), "terms=0"), (dict(group=2), "group=2"), (dict(group=1, divisor=0.0), "divisor=0"), (dict(reduce=3), "reduce=3"),
    (dict(reduce=-1), "reduce=-1"), (dict(ws_bytes=16), "workspace too small")])
def test_abi_refuses_before_launching(change, word):
    fwd, bwd, fmsg, bmsg = _abi_call(**change)
    assert (fwd, bwd) == (EINVAL, EINVAL), (fwd, bwd, fmsg, bmsg)
    assert word in fmsg and word in bmsg, (fmsg, bmsg)


@pytest.mark.parametrize("null", ["x", "y", "w2", "value", "reduced", "ws", "grad", "dx"])
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


def test_reduced_is_optional_without_a_reduction():
    """...but the call still stops at the short workspace, before any launch"""
    fwd, _, fmsg, _ = _abi_call(null="reduced", only="forward", reduce=0, ws_bytes=16)
    assert fwd == EINVAL and "workspace too small" in fmsg


def test_workspace_bytes_and_symbols():
    from pde_policylearning_amd import _lib
    nb = _lib.lib().fno_hs_loss_workspace_bytes
    assert nb(2, 3) >= (2 * 2 * 6 + 2 * 6) * 8          # six float64 sums a channel pair, (num_j, den_j) a sample
    assert nb(2, 4) == nb(2, 3) and nb(2, 5) > nb(2, 4) and nb(64, 1) > nb(2, 1) > 0
    assert nb(0, 3) == 0 and nb(2, 0) == 0 and nb(-1, 3) == 0
    assert all(n in _lib.EXPORTED_SYMBOLS for n in ("fno_hs_loss_workspace_bytes", "fno_hs_loss_forward", "fno_hs_loss_backward"))


def test_constants_are_the_headers():
    src = open(os.path.join(K.ROOT, "pde_policylearning_amd", "csrc", "k_hs_loss.h")).read()
    from pde_policylearning_amd import functional as F
    codes = {name: int(v) for name, v in re.findall(r"HS_REDUCE_(\w+) = (\d+)", src)}
    assert F.HS_REDUCE == {None: codes["NONE"], "sum": codes["SUM"], "mean": codes["MEAN"]}
    assert int(re.search(r"constexpr int HS_TERMS = (\d+);", src).group(1)) == F.HS_TERMS
    assert F.HS_GRIDS == K.GRIDS
    assert "atomic" not in src.replace("no atomics", "")
    assert '#include "k_pino_loss.h"' in src and "fft2_grid<" in src and not re.search(r"FNO_DEV void fft", src)      # reused, not copied


# ---------------------------------------------------------------------------------------------------------------------
# the class surface
# ---------------------------------------------------------------------------------------------------------------------
def test_constructor_attributes():
    from pde_policylearning_amd.libs.utilities3 import HsLoss
    h = HsLoss()
    assert (h.d, h.p, h.k, h.a, h.balanced, h.reduction, h.size_average) == (2, 2, 1, [1], False, True, True)
    h = HsLoss(d=3, k=2, a=[0.5, 0.25], group=True, size_average=False, reduction=False)
    assert (h.d, h.p, h.k, h.a, h.balanced, h.reduction, h.size_average) == (3, 2, 2, [0.5, 0.25], True, False, False)
    assert HsLoss(k=3).a == [1, 1, 1] and HsLoss(k=0, group=True).a == []
    with pytest.raises(AssertionError):
        HsLoss(d=0)
    with pytest.raises(NotImplementedError, match="p=3"):
        HsLoss(p=3)
    with pytest.raises(ValueError, match="the reference fails there"):
        HsLoss(k=0)
    x, y = K.make_inputs("white", (2, 32, 32, 3))
    assert judging.rel_err(HsLoss(reduction=False).rel(x, y), K.restated(x, y, torch.float32, 0, None, True, None)["samples"]) < 1e-6


def test_cpu_and_wrong_inputs_are_refused_by_name():
    from pde_policylearning_amd import functional as F
    from pde_policylearning_amd.libs.utilities3 import HsLoss
    x, y = torch.zeros(2, 32, 32, 3), torch.ones(2, 32, 32, 3)
    for call in (lambda: HsLoss()(x, y), lambda: HsLoss(k=2, group=True, reduction=False)(x, y), lambda: F.hs_loss(x, y)):
        with pytest.raises(RuntimeError, match="`x` must live on the GPU"):
            call()
    for shape in ((2, 48, 48), (2, 32, 64, 3), (2, 32)):
        with pytest.raises(RuntimeError, match=r"N = 32, 64, 128"):
            HsLoss()(torch.zeros(shape), torch.ones(shape))
    with pytest.raises(RuntimeError, match="`y` must be data"):
        HsLoss()(x, y.clone().requires_grad_(True))
    with pytest.raises(RuntimeError, match="`reduce` must be None, 'sum' or 'mean'"):
        F.hs_loss(x, y, reduce="max")
    with pytest.raises(RuntimeError, match="`a` must have a coefficient"):
        F.hs_loss(x, y, k=2, a=[1.0])
    for k in (-1, 1.5, None, True):
        with pytest.raises(RuntimeError, match="`k` must be a non-negative integer"):
            F.hs_loss(x, y, k=k)
    assert not F.hs_loss_supported(x) and not F.hs_loss_supported(torch.zeros(2, 48, 48))


def test_star_import_yields_the_scripts_names():
    """`from libs.utilities3 import *` (run_pde_observers.py:9, run_control.py:10) with the package's libs aliased as `libs`"""
    import sys
    import pde_policylearning_amd.libs as pkg
    from pde_policylearning_amd import trainer
    from pde_policylearning_amd.libs import utilities3
    names = ("libs", "libs.utilities3")
    saved = {k: sys.modules.get(k) for k in names}
    sys.modules["libs"], sys.modules["libs.utilities3"] = pkg, utilities3
    try:
        ns = {}
        exec("from libs.utilities3 import *", ns)
        assert ns["HsLoss"] is utilities3.HsLoss and ns["LpLoss"] is trainer.LpLoss
        assert ns["NormalizerGivenMeanStd"] is utilities3.NormalizerGivenMeanStd
        assert ns["count_params"](torch.nn.Linear(3, 4)) == 16
        assert ns["count_params"](torch.nn.ParameterList([torch.nn.Parameter(torch.zeros(2, 3, dtype=torch.cfloat))])) == 12
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
