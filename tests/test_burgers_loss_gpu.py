"""The Burgers residual loss (csrc/k_burgers_loss.h) on the GPU against the float64 restatement of tests/burgers_cases.py.
Every case first asserts from the launch log that only the Burgers kernels ran; every measured distance goes to
profiles/r20_burgers_errors.txt before anything is asserted."""
import pytest
import torch

from tests import burgers_cases as K
from tests.judging import dev, judge_budget, rel_err  # noqa: F401
from tests.step_tail_cases import same_bits

pytestmark = pytest.mark.gpu

FWD, BWD = ["k_burgers_fwd", "k_burgers_finish"], ["k_burgers_bwd"]
CASES = [(s, f, v) for s in K.SHAPES for f in K.families(s) for v in K.VISCS]


def evaluate(inp, visc, dev, g_u=K.IC_WEIGHT, g_f=1.0, backward=True):  # noqa: F811
    """{"loss_u", "loss_f", "field", "grad"} on the CPU and the launch records of one loss call (+ backward) and one
    burgers_residual call on the same input"""
    from pde_policylearning_amd import _lib
    from pde_policylearning_amd import functional as F
    u = inp["u"].to(dev).requires_grad_(backward)
    u0 = inp["u0"].to(dev)
    with _lib.launch_log() as log:
        loss_u, loss_f = F.burgers_loss(u, u0, visc)
        if backward:
            (g_u * loss_u + g_f * loss_f).backward()
        field = F.burgers_residual(u, visc)
        torch.cuda.synchronize()
    got = {"loss_u": loss_u.detach().cpu(), "loss_f": loss_f.detach().cpu(), "field": field.cpu()}
    if backward:
        got["grad"] = u.grad.cpu()
    return got, log.records


def assert_route(records, shape, backward=True):
    B, nt, nx = shape
    want = FWD + (BWD if backward else []) + FWD
    assert [r["name"] for r in records] == want, [r["name"] for r in records]
    tiles_f, tiles_b = -(-(nt - 2) // K.TJ), -(-nt // K.TJ)
    grids = [(B * tiles_f, 1, 1), (1, 1, 1)] + ([(B * tiles_b, 1, 1)] if backward else []) + [(B * tiles_f, 1, 1), (1, 1, 1)]
    assert [r["grid"] for r in records] == grids
    assert all(r["block"] == (256, 1, 1) for r in records)


@pytest.mark.parametrize("shape,family,visc", CASES, ids=[K.case_name(f, s, v).replace(" ", "_") for s, f, v in CASES])
def test_loss_vs_float64(dev, shape, family, visc):  # noqa: F811
    inp, ref64, ref32 = K.references(family, shape, visc)
    got, records = evaluate(inp, visc, dev)
    assert_route(records, shape)
    rows = K.loss_rows(got, ref64, ref32)
    section = K.case_name(family, shape, visc)
    if family == "smooth":
        # D2 r amplifies rounding in the high bins of a smooth field and the whole-tensor budget of du is loose there, so the
        # part of du_f in the first 16 bins is held to the same rule by itself (rows 1.. of du are du_f alone): measured
        # 1.1e-6 .. 1.3e-5 against a float32 yardstick of 1.3e-6 .. 1.4e-5, inside max(2e-6, 1.75 ref32) on every case
        rows.append(("du_f rows 1.., first 16 bins", rel_err(K.low_bins(got["grad"][:, 1:]), K.low_bins(ref64["grad"][:, 1:])),
                     rel_err(K.low_bins(ref32["grad"][:, 1:]), K.low_bins(ref64["grad"][:, 1:])), K.FLOOR))
    judge_budget(K.LOG, section, rows)


@pytest.mark.parametrize("g_u,g_f", [(0.7, -1.3), (2.0, 0.0), (0.0, 3.0)])
def test_upstream_gradients(dev, g_u, g_f):  # noqa: F811
    """non-unit, distinct upstream gradients; with one of them zero the other term's gradient is exact zeros where that
    term does not reach (loss_u reaches row 0 alone)"""
    shape, visc = (2, 34, 64), 0.01
    inp, ref64, ref32 = K.references("white", shape, visc, g_u, g_f)
    got, records = evaluate(inp, visc, dev, g_u, g_f)
    assert_route(records, shape)
    if g_f == 0.0:
        assert not bool(got["grad"][:, 1:].any()), "loss_u reaches row 0 only"
        rows = [("du row 0", rel_err(got["grad"][:, 0], ref64["grad"][:, 0]), rel_err(ref32["grad"][:, 0], ref64["grad"][:, 0]), K.FLOOR)]
    else:
        rows = [r for r in K.loss_rows(got, ref64, ref32) if r[0].startswith("du")]
    if g_u == 0.0:
        assert same_bits(got["grad"], evaluate(inp, visc, dev, 0.0, g_f)[0]["grad"])
        rows.append(("du row 0 (loss_f alone)", rel_err(got["grad"][:, 0], ref64["grad_f"][:, 0]),
                     rel_err(ref32["grad_f"][:, 0], ref64["grad_f"][:, 0]), K.FLOOR))
    judge_budget(K.LOG, f"upstream g_u={g_u:g} g_f={g_f:g} " + K.case_name("white", shape, visc), rows)


@pytest.mark.parametrize("shape", [(3, 11, 128), (2, 2 * K.TJ + 3, 64)])
def test_bitwise_repeatable_and_batch_independent(dev, shape):  # noqa: F811
    inp = K.make_inputs("white", shape)
    a, _ = evaluate(inp, 0.01, dev)
    b, _ = evaluate(inp, 0.01, dev)
    for k in ("loss_u", "loss_f", "field", "grad"):
        assert same_bits(a[k].reshape(-1), b[k].reshape(-1)), k
    for s in range(shape[0]):
        one, records = evaluate({k: v[s:s + 1] for k, v in inp.items()}, 0.01, dev, backward=False)
        assert_route(records, (1,) + shape[1:], backward=False)
        assert same_bits(one["field"][0], a["field"][s]), f"sample {s}"


def test_input_forms(dev):  # noqa: F811
    """(B, nt, nx, 1) as the model returns it, and a non-contiguous u (copied): the same bits"""
    from pde_policylearning_amd import functional as F
    from pde_policylearning_amd.libs.pino_utils.losses import FDM_Burgers, PINO_loss
    shape, visc = (2, 34, 64), 0.1
    inp = K.make_inputs("white", shape)
    base, _ = evaluate(inp, visc, dev)
    u0 = inp["u0"].to(dev)
    forms = {"trailing channel": inp["u"].to(dev).unsqueeze(-1),
             "transposed storage": inp["u"].to(dev).transpose(1, 2).contiguous().transpose(1, 2)}
    assert not forms["transposed storage"].is_contiguous()
    for name, u in forms.items():
        u = u.detach().requires_grad_(True)
        assert F.burgers_loss_supported(u)
        loss_u, loss_f = PINO_loss(u, u0, visc)
        (K.IC_WEIGHT * loss_u + loss_f).backward()
        assert u.grad.shape == u.shape, name
        assert same_bits(loss_u.cpu().reshape(1), base["loss_u"].reshape(1)) and same_bits(loss_f.cpu().reshape(1), base["loss_f"].reshape(1)), name
        assert same_bits(u.grad.cpu().reshape(shape), base["grad"]), name
        assert same_bits(FDM_Burgers(u.detach(), visc).cpu(), base["field"]), name
    assert not F.burgers_loss_supported(torch.zeros(2, 5, 48, device=dev))
    with pytest.raises(RuntimeError, match="nx=48"):
        F.burgers_loss(torch.zeros(2, 5, 48, device=dev), torch.zeros(2, 48, device=dev), visc)


def test_lploss_runs_on_the_engine(dev):  # noqa: F811
    from pde_policylearning_amd import _lib
    from pde_policylearning_amd.libs.pino_utils.losses import LpLoss
    x, y = K.make_inputs("white", (2, 34, 64))["u"].to(dev), K.make_inputs("smooth", (2, 34, 64))["u"].to(dev)
    for size_average in (True, False):
        with _lib.launch_log() as log:
            got = LpLoss(size_average=size_average)(x, y)
            torch.cuda.synchronize()
        assert log.records and all(r["name"].startswith("k_lploss") for r in log.records), [r["name"] for r in log.records]
        x64, y64 = x.double().cpu().reshape(2, -1), y.double().cpu().reshape(2, -1)
        per = (x64 - y64).norm(dim=1) / y64.norm(dim=1)
        want = per.mean() if size_average else per.sum()
        assert K.scalar_err(got, want) < K.FLOOR
