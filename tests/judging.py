"""How the tests decide that the engine is correct (a helper module, not a conftest): the two tolerance rules, the error
tables under profiles/ and the GPU fixture, each stated once.  Every measured distance is written to a table before anything
is asserted.

The float32-budget rule (`accept`, `judge_budget`): with err = a distance from the float64 evaluation on float64 copies of the
same float32 inputs,   err == 0 or err < max(floor, BUDGET_SLACK * err_ref32),   err_ref32 being the distance of the reference's
own float32 evaluation from the same float64 value.  A result that equals the float64 one exactly is inside any budget - there
0 < 1.75 * 0 would refuse a perfect answer.  NaN compares false and is refused.

The float64 floor rule (`bound`, `judge_floor`): the test measures a FLOOR on the CPU at the size at hand (a second float64
evaluation in another order, solver or precision) and the GPU gets   bound = min(16 * max(floor, resolution), CAP64),
resolution = eps = 2.2e-16 unless stated: two float64 evaluations of one quantity differ by eps unless they are bitwise equal;
1e-9 = cond * eps of the worst Poisson system (7e6 x 1.1e-16).

A feature's case module binds its table once at import - LOG = SectionLog(path) for a table of one block per case,
ROWS = RowLog("..._ERROR_LOG") for an appended one - builds rows and hands them to judge_budget / judge_floor; its GPU test
module takes the fixture with `from tests.judging import dev  # noqa: F401`."""
import os

import numpy as np
import pytest
import torch

TOL_Y = 1e-5
TOL_COMP = 5e-6
TOL_G = 1e-5          # north star: 1e-5 relative L2, gradients included (fp64 budget: test_fno_model_fp64_error_budget)

# Round 5 tried 1.25: five cases sit between 1.26 and 1.87 x the float32 oracle's own distance on tensors where that distance is
# itself above 1e-5 (dead-mode spectral weights, the 1e-6-scaled input: profiles/r05_hostile_errors.txt and
# r05_fullsize_budget_ratios.txt hold every achieved number).  On such tensors both float32 evaluations are draws of a
# conditioned quantity; the engine's split-precision GEMMs are ~1.5 x noisier there than torch's CPU float32, never 2 x.
# Round 6: 2.0 -> 1.75.  The largest ratios of profiles/r06_hostile_errors.txt on tensors whose float32-oracle error exceeds 5e-6
# are 1.70 / 1.69 / 1.52 (target_norm_1e-6: the SECOND-corner spectral weights of blocks 0-2, whose float32 oracle is itself
# 6e-6 .. 5e-5 from float64); every first-corner weight, skip weight and bias is below 1.2.
BUDGET_SLACK = 1.75
# The full-size comparison (tests/test_fullsize_gpu.py).  An ill-conditioned gradient is allowed this x the float32 oracle's own
# distance from float64.  Round 4 needed 2.0 for RNO2d: two float evaluations that decide a ReLU input of the regressor within
# rounding of zero differently differentiate different piecewise-linear functions, and every tensor upstream moves together by
# ~1e-5.  Round 5 compares MASK-CONDITIONED instead: the float64 / float32 oracles take the ENGINE's
# decisions for the regressor's two spectral layers (oracle/observers_oracle.py::ReluMasks; read off the engine's layer
# outputs), so all three evaluations differentiate the same function and what is left is arithmetic.
BUDGET_SLACK_FULLSIZE = 1.25

EPS64 = float(np.finfo(np.float64).eps)
CAP64 = 1e-9


def rel_err(a, ref64):
    """relative L2 of `a` against the float64 reference, evaluated in float64 where the reference lives"""
    b = ref64.detach().to(torch.float64)
    a = a.detach().to(device=b.device, dtype=torch.float64)
    den = float(b.norm())
    return float((a - b).norm()) / (den if den > 0 else 1.0)


def accept(err, err_ref32, floor, slack=BUDGET_SLACK):
    return err == 0.0 or err < max(floor, slack * err_ref32)


def bound(floor, resolution=EPS64):
    return min(16.0 * max(floor, resolution), CAP64)


class SectionLog:
    """an error table of one block per case: `## section` and its lines"""

    def __init__(self, path):
        self.path = path

    def replace(self, section, lines):
        """replace `section` by `lines`; the other blocks keep their order, a new or rewritten one goes last"""
        try:
            old = open(self.path).read().split("\n## ") if os.path.exists(self.path) else []
            keep = [b for b in old if b.strip() and not b.lstrip("# ").startswith(section + "\n")]
            body = "\n## ".join([b.lstrip("# ").rstrip("\n") for b in keep] + [section + "\n" + "\n".join(lines)])
            os.makedirs(os.path.dirname(self.path), exist_ok=True)
            with open(self.path, "w") as f:
                f.write("## " + body + "\n")
        except OSError as e:
            import warnings
            warnings.warn(f"the error log {self.path} could not be written ({e}); the figures of `{section}` are on stdout only")


class RowLog:
    """an error table of appended rows, in the file that the environment variable `env` names (unset: nothing is written)"""

    def __init__(self, env, widths=(52, 11)):
        self.env, self.widths = env, widths

    def write(self, case, quantity, text):
        path = os.environ.get(self.env)
        if path:
            with open(path, "a") as f:
                f.write(f"{case:<{self.widths[0]}s} {quantity:<{self.widths[1]}s} {text}\n")

    def row(self, case, quantity, who, err, err_ref32, limit, verdict):
        """limit: what the row was held to, as `floor 2.0e-06`; verdict: ok / FAIL / logged"""
        self.write(case, quantity, f"{who} {err:10.3e}   ref32 {err_ref32:10.3e}   {limit}   {verdict}")


def _judge(log, section, lines, ok):
    """print and log every line, then assert once"""
    for line in lines:
        print(section, line)
    log.replace(section, lines)
    bad = [line for line, good in zip(lines, ok) if not good]
    assert not bad, "\n".join([section] + bad)


def judge_budget(log, section, rows, who="engine", width=46):
    """rows: (name, err, err_ref32, floor) under the float32-budget rule.  Logs all, then asserts all."""
    ok = [accept(err, ref, floor) for _, err, ref, floor in rows]
    _judge(log, section, [f"{name:{width}s} {who} {err:10.3e}   ref32 {ref:10.3e}   floor {floor:7.1e}   {'ok' if good else 'MISS'}"
                          for (name, err, ref, floor), good in zip(rows, ok)], ok)


def rejected(rows):
    """names of the rows the float32-budget rule refuses (a planted fault must leave at least one)"""
    return [name for name, err, ref, floor in rows if not accept(err, ref, floor)]


def judge_floor(log, section, rows, width=52, plain_rule=False):
    """rows: (name, gpu distance, floor, resolution[, raw]) under the float64 floor rule, raw = relative to the entry's own
    magnitude where the distance is measured against a scale: the gpu figure, or with plain_rule the pair (gpu, floor).
    plain_rule: the bound of the plain rule (16 x the measured floor, the cap, no resolution) is recorded beside each figure,
    so that what the resolution and the scales loosen stays visible.  Logs all, then asserts all."""
    lines, ok = [], []
    for name, got, floor, res, *raw in rows:
        b = bound(floor, res)
        ok.append(got <= b)
        line = f"{name:{width}s} gpu {got:.3e}   floor {floor:.3e}   resolution {res:.3e}   bound {b:.3e}   {'ok' if ok[-1] else 'MISS'}"
        if plain_rule:
            line += f"   [plain rule: bound {min(16 * floor, CAP64):.3e}]"
            if raw:
                line += f"   [own magnitude: gpu {raw[0][0]:.3e}   floor {raw[0][1]:.3e}   plain-rule bound {min(16 * raw[0][1], CAP64):.3e}]"
        elif raw:
            line += f"   [own magnitude: gpu {raw[0]:.3e}]"
        lines.append(line)
    _judge(log, section, lines, ok)


@pytest.fixture(scope="module")
def dev():
    """cuda:0 with the library loaded.  The cap on torch's CPU threads is process-global; setting it in every GPU module keeps
    the CPU oracles from depending on which module ran first."""
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from pde_policylearning_amd import _lib
    _lib.lib()   # fails loudly when the HIP library is absent
    torch.set_num_threads(min(torch.get_num_threads(), 16))
    return torch.device("cuda:0")
