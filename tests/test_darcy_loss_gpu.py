"""The Darcy residual loss (csrc/k_darcy_loss.h) on the GPU against the float64 restatement of tests/darcy_cases.py.
Every case first asserts from the launch log that only the Darcy kernels ran; every measured distance goes to
profiles/r21_darcy_errors.txt before anything is asserted."""
import pytest
import torch

from tests import darcy_cases as K
from tests.judging import dev, judge_budget, rel_err  # noqa: F401
from tests.step_tail_cases import same_bits

pytestmark = pytest.mark.gpu

FWD, BWD = ["k_darcy_fwd", "k_darcy_finish"], ["k_darcy_bwd"]
CASES = [(s, f) for s in K.SHAPES for f in K.families(s)]
FORMS = [(y, mol) for y in (True, False) for mol in (True, False)]
FORM_IDS = [("y" if y else "no-y") + ("_mol" if mol else "_no-mol") for y, mol in FORMS]


def evaluate(inp, dev, mol=True, y=True, g_data=K.DATA_WEIGHT, g_f=1.0, backward=True):  # noqa: F811
    """{"loss_f", "field"[, "loss_data", "grad"]} on the CPU and the launch records of one loss call (+ backward) and one
    darcy_residual call on the same input"""
    from pde_policylearning_amd import _lib
    from pde_policylearning_amd import functional as F
    out, a, yt, m = (None if t is None else t.to(dev) for t in K.operands(inp, mol, y))
    out.requires_grad_(backward)
    with _lib.launch_log() as log:
        res = F.darcy_loss(out, a, yt, m)
        loss_data, loss_f = res if y else (None, res)
        if backward:
            (g_f * loss_f + (g_data * loss_data if y else 0.0)).backward()
        field = F.darcy_residual(out, a, m)
        torch.cuda.synchronize()
    got = {"loss_f": loss_f.detach().cpu(), "field": field.cpu()}
    if y:
        got["loss_data"] = loss_data.detach().cpu()
    if backward:
        got["grad"] = out.grad.cpu()
    return got, log.records


def assert_route(records, shape, backward=True):
    B, S = shape
    want = FWD + (BWD if backward else []) + FWD
    assert [r["name"] for r in records] == want, [r["name"] for r in records]
    tiles = -(-(S - 4) // K.T)
    grids = [(B * tiles * tiles, 1, 1), (1, 1, 1)] + ([(B * tiles * tiles, 1, 1)] if backward else []) + [(B * tiles * tiles, 1, 1), (1, 1, 1)]
    assert [r["grid"] for r in records] == grids
    assert all(r["block"] == (256, 1, 1) for r in records)


@pytest.mark.parametrize("shape,family", CASES, ids=[K.case_name(f, s).replace(" ", "_") for s, f in CASES])
def test_loss_vs_float64(dev, shape, family):  # noqa: F811
    """the full form: mollifier and data term, dout of loss_f + 5 loss_data"""
    inp, ref64, ref32 = K.references(family, shape, mol=True, y=True)
    got, records = evaluate(inp, dev)
    assert_route(records, shape)
    judge_budget(K.LOG, K.case_name(family, shape, mol=True), K.loss_rows(got, ref64, ref32))


@pytest.mark.parametrize("y,mol", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("g_data,g_f", [(0.7, -1.3), (2.0, 0.0), (0.0, 3.0)])
def test_upstream_gradients(dev, g_data, g_f, y, mol):  # noqa: F811
    """non-unit, distinct upstream gradients; either of them zero.  With g_data = 0 (or no data term) the four 2 x 2 corner
    blocks, which the equation term never reaches, are exact zeros."""
    shape, family = (2, 2 * K.T + 5), "white"
    inp, ref64, ref32 = K.references(family, shape, mol, y, g_data, g_f)
    got, records = evaluate(inp, dev, mol, y, g_data, g_f)
    assert_route(records, shape)
    section = f"upstream g_data={g_data:g} g_f={g_f:g} " + K.case_name(family, shape, mol, y)
    if g_data == 0.0 or not y:
        assert not bool(K.corner_blocks(got["grad"]).any()), "the equation term does not reach the corner blocks"
    if g_f == 0.0 and not y:
        assert not bool(got["grad"].any()), "no term is left"
        return
    rows = [r for r in K.loss_rows(got, ref64, ref32) if r[0].startswith("dout")]
    judge_budget(K.LOG, section, rows)


@pytest.mark.parametrize("y,mol", FORMS, ids=FORM_IDS)
def test_forms_vs_float64(dev, y, mol):  # noqa: F811
    """with and without the data term and the mollifier, on the workload's grid in both families"""
    for family in ("white", "darcy"):
        shape = (2, 61)
        inp, ref64, ref32 = K.references(family, shape, mol, y)
        got, records = evaluate(inp, dev, mol, y)
        assert_route(records, shape)
        judge_budget(K.LOG, "forms " + K.case_name(family, shape, mol, y), K.loss_rows(got, ref64, ref32))


@pytest.mark.parametrize("y,mol", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("shape", [(3, 37), (2, 2 * K.T + 5)])
def test_bitwise_repeatable_and_batch_independent(dev, shape, y, mol):  # noqa: F811
    inp = K.make_inputs("white", shape)
    a, _ = evaluate(inp, dev, mol, y)
    b, _ = evaluate(inp, dev, mol, y)
    for k in a:
        assert same_bits(a[k].reshape(-1), b[k].reshape(-1)), k
    for s in range(shape[0]):
        one, records = evaluate({k: (v if k == "mol" else v[s:s + 1]) for k, v in inp.items()}, dev, mol, y, backward=False)
        assert_route(records, (1,) + shape[1:], backward=False)
        assert same_bits(one["field"][0], a["field"][s]), f"sample {s}"


@pytest.mark.parametrize("y,mol", FORMS, ids=FORM_IDS)
def test_input_forms(dev, y, mol):  # noqa: F811
    """(B, S, S, 1) as the model returns it, a non-contiguous u (copied) and a = x[..., 0] (copied): the same bits"""
    from pde_policylearning_amd import functional as F
    shape = (2, 37)
    inp = K.make_inputs("white", shape)
    base, _ = evaluate(inp, dev, mol, y)
    out, a, yt, m = (None if t is None else t.to(dev) for t in K.operands(inp, mol, y))
    x = torch.stack([a, torch.zeros_like(a), torch.ones_like(a)], dim=-1)
    assert not x[..., 0].is_contiguous()
    forms = {"trailing channel": out.unsqueeze(-1), "transposed storage": out.transpose(1, 2).contiguous().transpose(1, 2)}
    assert not forms["transposed storage"].is_contiguous()
    for name, u in forms.items():
        u = u.detach().requires_grad_(True)
        assert F.darcy_loss_supported(u)
        res = F.darcy_loss(u, x[..., 0], yt, m)
        loss_data, loss_f = res if y else (None, res)
        (loss_f + (K.DATA_WEIGHT * loss_data if y else 0.0)).backward()
        assert u.grad.shape == u.shape, name
        assert same_bits(loss_f.detach().cpu().reshape(1), base["loss_f"].reshape(1)), name
        if y:
            assert same_bits(loss_data.detach().cpu().reshape(1), base["loss_data"].reshape(1)), name
        assert same_bits(u.grad.cpu().reshape(base["grad"].shape), base["grad"]), name
        assert same_bits(F.darcy_residual(u.detach(), x[..., 0], m).cpu(), base["field"]), name


def test_reference_surface(dev):  # noqa: F811
    """losses.FDM_Darcy / darcy_loss (no mollifier, no data term) are the fused call's bits; refusals on the GPU"""
    from pde_policylearning_amd import functional as F
    from pde_policylearning_amd.libs.pino_utils.losses import FDM_Darcy, darcy_loss
    inp = K.make_inputs("darcy", (2, 61))
    base, _ = evaluate(inp, dev, mol=False, y=False, backward=False)
    u, a = inp["u"].to(dev), inp["a"].to(dev)
    assert same_bits(darcy_loss(u.unsqueeze(-1), a.unsqueeze(-1)).cpu().reshape(1), base["loss_f"].reshape(1))
    assert same_bits(FDM_Darcy(u, a).cpu(), base["field"])
    assert not F.darcy_loss_supported(torch.zeros(2, 4, 4, device=dev)) and not F.darcy_loss_supported(torch.zeros(2, 7, 8, device=dev))
    with pytest.raises(RuntimeError, match="S=4"):
        F.darcy_loss(torch.zeros(2, 4, 4, device=dev), torch.zeros(2, 4, 4, device=dev))
    with pytest.raises(RuntimeError, match="square"):
        F.darcy_loss(torch.zeros(2, 7, 8, device=dev), torch.zeros(2, 7, 8, device=dev))


def test_zero_residual_gives_a_zero_gradient(dev):  # noqa: F811
    """a sample whose residual norm is exactly zero (a = 0 and Du = 0 cannot give it: Du - 1 = -1; so out such that the stored
    field is exactly 1 is needed - a = 1, pred = -x^2 / 2 on S = 5 is exact in float32) contributes zeros, not NaN"""
    from pde_policylearning_amd import functional as F
    S = 5
    xs = torch.arange(S, dtype=torch.float32) / (S - 1)
    u = (-(xs * xs) / 2)[None, :, None].repeat(1, 1, S).to(dev).requires_grad_(True)
    a = torch.ones(1, S, S, device=dev)
    field = F.darcy_residual(u.detach(), a)
    assert float(field.reshape(-1)[0]) == 1.0, "the construction is exact in float32"
    loss_f = F.darcy_loss(u, a)
    loss_f.backward()
    assert float(loss_f.detach()) == 0.0 and not bool(u.grad.any()) and bool(torch.isfinite(u.grad).all())
