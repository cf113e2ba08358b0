"""CPU self-test of the PINO residual-loss comparison (tests/pino_loss_cases.py): on the budget cases of
tests/test_pino_loss_gpu.py
  - the float32 oracle alone stays under the cap below which a row is judged at all (so no judged row can turn into a
    logged one unnoticed),
  - a float32 numpy restatement of the kernels' arithmetic (radix-2 DIF / DIT, float32 twiddles, Hermitian-extended
    multipliers, 1 / n^2 after the inverse) passes every judged forward row - a correct float32 kernel can meet the budget,
  - five faults planted in a float64 copy of the oracle - where the fault is the only error there is - are refused by the
    gradient rows of a named case, and the case that cannot see a fault is named too."""
import pytest
import torch

from oracle import pino_loss_oracle as P
from tests import pino_loss_cases as C

BUDGET_CASES = [(fam, d, n, B, nt) for n, B, nt in C.BUDGET_SHAPES for fam, d in C.budget_families(n)]


def _id(c):
    fam, d, n, B, nt = c
    return C.case_name(fam, d, n, B, nt).replace(" ", "_")


def test_references_are_the_oracle_itself():
    """ref64 / ref32 are oracle.pino_loss, bit for bit; ref32n differs from ref32 in the norms alone"""
    inp, ref64, ref32, ref32n = C.references("white", None, 32, 3, 3)
    for ref, dtype in ((ref64, torch.float64), (ref32, torch.float32)):
        lic, lf = P.pino_loss(inp["u"].to(dtype), inp["u0"].to(dtype), inp["f"].to(dtype), inp["visc"].to(dtype), C.T_INTERVAL)
        assert float(lic) == float(ref["loss_ic"]) and float(lf) == float(ref["loss_f"]) and ref["grad"].dtype == dtype
    assert torch.equal(ref32n["field"], ref32["field"]) and ref32n["grad"].dtype == torch.float32
    assert C.scalar_err(ref32n["loss_f"], ref32["loss_f"]) < 1e-6


@pytest.mark.parametrize("case", BUDGET_CASES, ids=_id)
def test_float32_oracle_stays_under_the_cap(case):
    """every quantity of every judged case: err_ref32 < 0.1 (the yardstick of the reduction row is the engine's own field
    and is at rounding level by construction)"""
    fam, d, n, B, nt = case
    _, ref64, ref32, ref32n = C.references(fam, d, n, B, nt)
    errs = {"field": C.rel_err(ref32["field"], ref64["field"]),
            "field/plane": C.worst_slice_err(ref32["field"], ref64["field"], (2, 3)),
            "max|e|/rms": C.max_over_rms(ref32["field"], ref64["field"]),
            "loss_ic": C.scalar_err(ref32["loss_ic"], ref64["loss_ic"]),
            "grad": C.rel_err(ref32n["grad"], ref64["grad"]),
            "grad/level": C.worst_slice_err(ref32n["grad"], ref64["grad"], (0, 1, 2))}
    assert all(e < C.CAP for e in errs.values()), errs


@pytest.mark.parametrize("case", BUDGET_CASES, ids=_id)
def test_restated_forward_in_float32_stays_in_budget(case):
    fam, d, n, B, nt = case
    inp, ref64, ref32, _ = C.references(fam, d, n, B, nt)
    bad = C.forward_failures(C.case_name(fam, d, n, B, nt), C.restated_forward(inp), ref32, ref64, inp["f"], who="restated")
    assert not bad, "\n".join(bad)


def test_restated_slab_order_equals_plane_order_in_budget():
    """the inverse transform's two orders (y then x in one workgroup, x then y through the slabs) are both in budget at 128,
    the grid fno_debug_pino_twopass routes either way"""
    inp, ref64, ref32, _ = C.references("white", None, 128, 2, 4)
    for slab in (False, True):
        bad = C.forward_failures(f"pino white n=128 slab={slab}", C.restated_forward(inp, slab=slab), ref32, ref64, inp["f"], who="restated")
        assert not bad, "\n".join(bad)


def test_const_in_space_restated_is_exact():
    """the restatement reproduces the closed form the GPU test holds the engine to, bit for bit"""
    for n in (32, 256):
        inp = C.make_inputs("const", 2, n, 5)
        assert C.same_bits(C.restated_forward(inp, 0.37)["field"], C.const_expected(inp, 0.37))


# ---------------------------------------------------------------------------------------------------------------------
# planted faults, each in a float64 copy of the oracle: the fault is the whole error
# ---------------------------------------------------------------------------------------------------------------------
def _planted(fault, fam, d, n, B, nt, t_interval=C.T_INTERVAL):
    inp, ref64, ref32, ref32n = C.references(fam, d, n, B, nt, t_interval)
    got = C.oracle_eval(inp, torch.float64, t_interval, fault=fault)
    name = f"{fault}: " + C.case_name(fam, d, n, B, nt, t_interval)
    bad = C.forward_failures(name, got, ref32, ref64, inp["f"], who="planted") \
        + C.grad_failures(name, got["grad"], ref32n, ref32, ref64, who="planted")
    return {b.split(":")[1].split()[-1] for b in bad}, C.rel_err(got["grad"], ref64["grad"])


@pytest.mark.parametrize("n,B,nt", C.BUDGET_SHAPES)
def test_planted_nonlinear_scale_is_refused(n, B, nt):
    """(a) u . grad(w) times 1.001: refused by the gradient of every white case (1.3e-5 .. 3.3e-5 against a floor of 2e-6).
    On steady(0.1) it moves the gradient by 1e-3, which is refused at 32 and 64; at 128 and 256 the float32 oracle itself is
    1.4e-3 / 3.9e-3 from float64 there, so 1.75 times that lets the fault through - near the solution white noise is the
    sharper probe of the nonlinear term, not the near-steady family."""
    blamed, g = _planted("nonlinear", "white", None, n, B, nt)
    assert {"grad", "grad/level"} <= blamed and 1e-5 < g < 5e-5, (blamed, g)
    blamed, g = _planted("nonlinear", "steady", 1e-1, n, B, nt)
    assert 5e-4 < g < 2e-3 and (n > 64 or {"grad", "grad/level"} <= blamed), (blamed, g)


@pytest.mark.parametrize("n,B,nt", C.BUDGET_SHAPES)
def test_planted_nyquist_row_is_refused_on_white(n, B, nt):
    """(b) the row kx = -n/2 missing from u_y: refused by every white case.  The smooth family (spectrum |k|^-3) has next to
    nothing in that row from 128 points on (gradient moved by less than 3e-6) and lets it through - which is why white noise
    stays in the table."""
    blamed, g = _planted("nyquist_row", "white", None, n, B, nt)
    assert {"field", "grad", "grad/level"} <= blamed and g > 1e-4, (blamed, g)
    if n >= 128:
        blamed, g = _planted("nyquist_row", "smooth", None, n, B, nt)
        assert not blamed and g < 3e-6, (blamed, g)


def test_planted_chunk_viscosity_is_refused():
    """(c) planes >= 64 take visc[0]: refused by the (2, 35) slab case (66 planes, the last two of sample 1), at the 128
    grid that fno_debug_pino_twopass routes through the slabs; no budget case has a 65th plane"""
    blamed, _ = _planted("visc_chunk", "white", None, 128, 2, 35, C.SLAB_T_INTERVAL)
    assert {"field", "field/plane", "grad", "grad/level"} <= blamed, blamed
    for n, B, nt in C.BUDGET_SHAPES:
        assert not _planted("visc_chunk", "white", None, n, B, nt)[0]


@pytest.mark.parametrize("n,B,nt", C.BUDGET_SHAPES)
def test_planted_last_level_adjoint_is_refused(n, B, nt):
    """(d) level T - 1 gets no gradient from the central difference: a backward fault - no forward row moves, the worst
    time level is wrong by 100 %"""
    blamed, _ = _planted("last_level_adjoint", "white", None, n, B, nt)
    assert blamed == {"grad", "grad/level"}, blamed


@pytest.mark.parametrize("n,B,nt", C.BUDGET_SHAPES)
def test_planted_dt_slip_is_refused(n, B, nt):
    """(e) w_t times T / (T - 1): refused by field and gradient of the smooth cases, where w_t is not drowned by the
    viscous term"""
    blamed, _ = _planted("dt_slip", "smooth", None, n, B, nt)
    assert {"field", "field/plane", "grad", "grad/level"} <= blamed, blamed


def test_comparison_rules():
    assert C.judge("c", "x", 1e-7, 1e-7) is None and C.judge("c", "x", 3e-6, 1e-7) is not None
    assert C.judge("c", "x", 0.3, 0.2) is not None                      # a reference above the cap is a failure by itself
    assert C.judge("c", "x", 1.0, 1e-7, log_only=True) is None
    assert C.judge("c", "x", float("nan"), 1e-7) is not None
