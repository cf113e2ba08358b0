"""tests/judging.py held to its own statement: the two rules on literal tables chosen from the formulas (no kernel is
involved), the two table writers, the judges, and that the case modules of the CPU suite learn the rules without importing the
GPU parity module."""
import os
import subprocess
import sys

import pytest

from tests import judging as J

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")


@pytest.mark.parametrize("err,ref,floor,slack,want", [
    (2e-6, 0.0, 2e-6, None, False),                 # exactly at the floor: the comparison is strict
    (1.9999e-6, 0.0, 2e-6, None, True),             # just below it
    (0.0, 0.0, 0.0, None, True),                    # an exact result is inside any budget
    (1e-30, 0.0, 0.0, None, False),                 # but nothing else is inside an empty one
    (NAN, 1.0, 1.0, None, False),
    (1e-7, NAN, 0.0, None, False),
    (1.74e-7, 1e-7, 0.0, None, True),               # 1.75 x the reference on either side
    (1.76e-7, 1e-7, 0.0, None, False),
    (1.76e-7, 1e-7, 2e-6, None, True),              # the larger of the two limits holds
    (1.24e-7, 1e-7, 0.0, J.BUDGET_SLACK_FULLSIZE, True),
    (1.26e-7, 1e-7, 0.0, J.BUDGET_SLACK_FULLSIZE, False),
])
def test_budget_rule(err, ref, floor, slack, want):
    assert (J.BUDGET_SLACK, J.BUDGET_SLACK_FULLSIZE, J.TOL_Y, J.TOL_G, J.TOL_COMP) == (1.75, 1.25, 1e-5, 1e-5, 5e-6)
    got = J.accept(err, ref, floor) if slack is None else J.accept(err, ref, floor, slack)
    assert bool(got) is want


def test_floor_rule():
    assert J.EPS64 == 2.0 ** -52 and J.CAP64 == 1e-9
    assert J.bound(0.0) == J.bound(1e-17) == 16 * 2.0 ** -52                  # a floor below the resolution of the format
    assert J.bound(1e-12) == 16.0 * 1e-12
    assert J.bound(1e-10) == J.bound(1.0) == 1e-9                             # 16 x floor above the cap
    assert J.bound(6e-11) == 16.0 * 6e-11 < 1e-9                              # and just below it
    assert J.bound(1e-15, resolution=1e-13) == 16.0 * 1e-13
    assert J.bound(1e-12, resolution=1e-13) == 16.0 * 1e-12
    assert J.bound(0.0, resolution=1e-3) == 1e-9


def test_section_log(tmp_path):
    a, b = J.SectionLog(str(tmp_path / "sub" / "a.txt")), J.SectionLog(str(tmp_path / "b.txt"))
    a.replace("one", ["1", "2"])
    a.replace("one more", ["3"])                    # a section whose name begins like another's
    a.replace("two", ["4"])
    b.replace("one", ["other"])
    assert open(a.path).read() == "## one\n1\n2\n## one more\n3\n## two\n4\n"
    a.replace("one", ["5"])                         # the others keep their order, the rewritten block goes last
    assert open(a.path).read() == "## one more\n3\n## two\n4\n## one\n5\n"
    assert open(b.path).read() == "## one\nother\n"
    (tmp_path / "dir").mkdir()
    with pytest.warns(UserWarning, match="could not be written"):
        J.SectionLog(str(tmp_path / "dir")).replace("one", ["1"])


def test_row_log(tmp_path, monkeypatch):
    log = J.RowLog("JUDGING_TEST_LOG", widths=(6, 4))
    monkeypatch.delenv("JUDGING_TEST_LOG", raising=False)
    log.row("case", "q", "engine", 1e-7, 2e-7, "floor 2.0e-06", "ok")             # unset: nothing is written
    monkeypatch.setenv("JUDGING_TEST_LOG", str(tmp_path / "rows.txt"))
    log.row("case", "q", "engine", 1e-7, 2e-7, "floor 2.0e-06", "ok")
    log.write("case", "q", "free text")
    assert open(tmp_path / "rows.txt").read() == ("case   q    engine  1.000e-07   ref32  2.000e-07   floor 2.0e-06   ok\n"
                                                  "case   q    free text\n")


def test_judges_log_every_row_then_name_the_bad_one(tmp_path):
    log = J.SectionLog(str(tmp_path / "t.txt"))
    rows = [("good", 1e-7, 1e-7, 0.0), ("bad", 1e-6, 1e-7, 0.0), ("exact", 0.0, 0.0, 0.0)]
    assert J.rejected(rows) == ["bad"]
    with pytest.raises(AssertionError, match="budget case\nbad ") as e:
        J.judge_budget(log, "budget case", rows, who="restated", width=8)
    assert "good" not in str(e.value) and "exact" not in str(e.value)
    assert open(log.path).read() == ("## budget case\n"
                                     "good     restated  1.000e-07   ref32  1.000e-07   floor 0.0e+00   ok\n"
                                     "bad      restated  1.000e-06   ref32  1.000e-07   floor 0.0e+00   MISS\n"
                                     "exact    restated  0.000e+00   ref32  0.000e+00   floor 0.0e+00   ok\n")
    J.judge_budget(log, "budget clean", rows[::2])

    rows = [("good", 1e-12, 1e-13, J.EPS64, 2e-12), ("bad", 1e-9, 6.25e-12, J.EPS64), ("nan", NAN, 1e-13, J.EPS64)]
    with pytest.raises(AssertionError, match="floor case\nbad ") as e:
        J.judge_floor(log, "floor case", rows, width=5)
    assert "good" not in str(e.value) and "nan " in str(e.value)
    assert open(log.path).read().split("## floor case\n")[1] == (
        "good  gpu 1.000e-12   floor 1.000e-13   resolution 2.220e-16   bound 1.600e-12   ok   [own magnitude: gpu 2.000e-12]\n"
        "bad   gpu 1.000e-09   floor 6.250e-12   resolution 2.220e-16   bound 1.000e-10   MISS\n"
        "nan   gpu nan   floor 1.000e-13   resolution 2.220e-16   bound 1.600e-12   MISS\n")
    rows = [("good", 1e-12, 1e-13, 1e-12, (2e-12, 1e-12)), ("bad", 1e-9, 6.25e-12, J.EPS64)]
    with pytest.raises(AssertionError, match="plain case\nbad "):
        J.judge_floor(log, "plain case", rows, width=5, plain_rule=True)
    assert open(log.path).read().split("## plain case\n")[1] == (
        "good  gpu 1.000e-12   floor 1.000e-13   resolution 1.000e-12   bound 1.600e-11   ok   [plain rule: bound 1.600e-12]"
        "   [own magnitude: gpu 2.000e-12   floor 1.000e-12   plain-rule bound 1.600e-11]\n"
        "bad   gpu 1.000e-09   floor 6.250e-12   resolution 2.220e-16   bound 1.000e-10   MISS   [plain rule: bound 1.000e-10]\n")


def test_case_modules_do_not_import_the_gpu_parity_module():
    code = ("import sys; "
            "from tests import step_tail_cases, pino_loss_cases, spec_conv_cases, action_opt_cases, policy_opt_cases, judging; "
            "bad = [m for m in sys.modules if m.startswith('tests.test_')]; assert not bad, bad")
    subprocess.run([sys.executable, "-c", code], cwd=ROOT, check=True)
