"""CPU self-test of the step-tail comparison (tests/step_tail_cases.py), as tests/test_hygiene_harness.py is of the hygiene
harness: on every sweep case small enough for the host, a float32 torch restatement of the kernels' arithmetic (another
operation order than torch's own float32, no fused multiply-adds) stays inside the budget the GPU module holds the engine
to - so the floors, and for Adam the budget alone, can be met by a correct float32 implementation - and three planted
faults, each a few lines in the restatements, are refused by the same comparison:
  the negative SELU branch as alpha (exp(s) - 1) / alpha exp(s) - alpha     at sigma <= 1e-2
  Adam's bias corrections taken at step t - 1
  a loss that drops every sample with index >= 256
Left to the GPU module: the gate shapes above one grid sweep + 4 elements and Adam above S + 1 elements (S taken for
256 compute units here)."""
import pytest
import torch

from tests import step_tail_cases as T

CPU = torch.device("cpu")
N_CU = 256
GATE_CASES = [c for c in T.gate_cases() if not c["big"]]
LOSS_CASES = T.loss_cases()
ADAM_CASES = [T.adam_resolve(c, N_CU) for c in T.adam_cases(cpu=True)]


def _ids(cases):
    return [c["name"].replace(" ", "_") for c in cases]


def _gates(case, fault=False):
    t, g_hn, g_rh = T.gate_inputs(case, CPU)
    ref64, ref32 = T.gates_torch(t, g_hn, g_rh, torch.float64), T.gates_torch(t, g_hn, g_rh, torch.float32)
    return T.judge_all(case["name"], T.gates_restated(t, g_hn, g_rh, fault=fault), ref32, ref64, T.gate_floor,
                       who="planted" if fault else "restated")


@pytest.mark.parametrize("case", GATE_CASES, ids=_ids(GATE_CASES))
def test_gates_restated_in_float32_stay_in_budget(case):
    assert not _gates(case)


@pytest.mark.parametrize("case", [c for c in GATE_CASES if c["sigma"] <= 1e-2], ids=lambda c: c["name"].replace(" ", "_"))
def test_planted_selu_cancellation_is_refused(case):
    """Refused through d(a7) = d(a8), which the backward's recomputed selu feeds (2.2e-6 at sigma = 1e-2, 2.2e-5 at 1e-3), and
    at sigma = 1e-3 through h' as well (1.2e-5; at 1e-2 its 1.4e-6 is under the 2e-6 floor); nothing else is blamed."""
    bad = _gates(case, fault=True)
    blamed = {b.split(":")[0].split()[-1] for b in bad}
    assert {"d_a7", "d_a8"} <= blamed <= {"hn", "d_a7", "d_a8", "d_b4"}, bad
    assert "hn" in blamed or case["sigma"] > 1e-3, bad


def _loss(case, drop_from=None):
    inp = T.loss_inputs(case, CPU)
    ref64, ref32 = T.loss_torch(case, *inp, torch.float64), T.loss_torch(case, *inp, torch.float32)
    return T.judge_all(case["name"], T.loss_restated(case, *inp, drop_from=drop_from), ref32, ref64, lambda k: T.FLOOR_LOSS,
                       who="planted" if drop_from else "restated")


@pytest.mark.parametrize("case", LOSS_CASES, ids=_ids(LOSS_CASES))
def test_loss_restated_in_float32_stays_in_budget(case):
    assert not _loss(case)


@pytest.mark.parametrize("case", [c for c in LOSS_CASES if c["B"] > 256], ids=lambda c: c["name"].replace(" ", "_"))
def test_planted_dropped_samples_are_refused(case):
    bad = "\n".join(_loss(case, drop_from=256))
    assert " loss:" in bad and " dpred:" in bad, bad


def test_dropping_from_256_is_invisible_below_257_samples():
    """... which is why the sweep has B = 257 and B = 1000: the fault passes every case of the earlier size"""
    for case in LOSS_CASES:
        if case["B"] <= 256 and case["n"] <= 4097:
            assert not _loss(case, drop_from=256)


def test_scale_property_holds_for_the_restated_loss():
    case = dict(size_average=False, gout=None)

    def run(pred, tgt):
        out = T.loss_restated(case, pred, tgt, None, None)
        return out["loss"], out["dpred"]
    assert not T.scale_property_failures(run, CPU)


def _adam(case, shift=0):
    p0, grad_of = T.adam_inputs(case, CPU)
    ref64, ref32 = T.adam_torch(case, p0, grad_of, torch.float64), T.adam_torch(case, p0, grad_of, torch.float32)
    return T.adam_failures(case, T.adam_restated(case, p0, grad_of, bias_step_shift=shift), ref32, ref64,
                           who="planted" if shift else "restated")


@pytest.mark.parametrize("case", ADAM_CASES, ids=_ids(ADAM_CASES))
def test_adam_restated_in_float32_stays_in_budget(case):
    assert not _adam(case)


@pytest.mark.parametrize("case", [c for c in ADAM_CASES if c["n"] == 1027 and (c["gscale"] or c["wd"])],
                         ids=lambda c: c["name"].replace(" ", "_"))
def test_planted_stale_bias_correction_is_refused(case):
    """(not the all-zero gradient without weight decay: nothing moves there, with any bias correction).  The fault starts at
    the second step and never touches the moments: the parameters after 20 steps are blamed, at either parameter scale, and
    nothing else is - without weight decay, which feeds the wrong parameters back into the moments."""
    bad = _adam(case, shift=-1)
    blamed = {" ".join(b.split(":")[0].split()[-3:]) for b in bad}
    assert "step 20 p" in blamed and not any(b.startswith("step 1 ") for b in blamed), bad
    assert case["wd"] or blamed == {"step 20 p"}, bad


def test_comparison_itself():
    assert T.accept(0.0, 0.0, 0.0) and T.accept(1.7e-7, 1e-7, 0.0) and T.accept(1.9e-6, 0.0, 2e-6)
    assert not T.accept(1.8e-7, 1e-7, 0.0) and not T.accept(float("nan"), 1.0, 1.0) and not T.accept(2e-6, 1e-8, 2e-6)
    assert not T.accept(1e-30, 0.0, 0.0)
