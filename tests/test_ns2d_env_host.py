"""Host side of NSControlEnv2D (no GPU): the numpy restatement of tests/ns2d_cases.py against the values the reference's own
class produced (tests/golden/ns2d_reference.npz, tools/make_ns2d_golden.py), the run plan of an `env_name: NSControlEnv2D` YAML
and the refusals that need no device."""
import argparse
import os

import numpy as np
import pytest

from tests import ns2d_cases as N
from tests.util import GOLDEN, load_golden

# settings data of the reference's configs/python_env_rno.yaml (keys and values, comments dropped), kept as a fixture
PYTHON_ENV_RNO = open(os.path.join(GOLDEN, "python_env_rno.yaml")).read()

TOL = 4 * N.EPS


@pytest.fixture(scope="module")
def golden():
    return load_golden("ns2d_reference")


def _close(got, want, what):
    d = N.rel(got, want)
    assert d <= TOL, f"{what}: {d:.3e} of max|field| (allowed {TOL:.3e})"


def _check_solve(r, z, what):
    for k in ("p", "u", "v"):
        _close(r[k], z[k], f"{what} {k}")
    _close(r["bulk_v"], z["bulk_v"], f"{what} bulk_v")
    assert r["steps"] == int(z["steps"]), f"{what}: {r['steps']} steps, the reference took {int(z['steps'])}"


@pytest.mark.parametrize("ny,nx", N.CAPPED_GRIDS)
def test_restated_capped_solve_matches_reference(golden, ny, nx):
    states, bcs = N.capped_case(ny, nx)
    for b, (st, bc) in enumerate(zip(states, bcs)):
        r = N.solve(N.Grid(ny, nx), st, bc, 3, N.CAPPED_NU[b], N.CAPPED_F[b])
        _check_solve(r, golden[f"capped_{ny}x{nx}_{b}"], f"{ny}x{nx} environment {b}")
        assert r["status"] == ("max_step" if r["steps"] == 3 else "converged")      # F = 0 leaves after one step: udiff < 0


@pytest.mark.parametrize("tag,g,start", [("conv_9x12", N.Grid(9, 12), N.small_start), ("conv_41x41", N.Grid(41, 41), N.seeded_start)])
def test_restated_converged_solve_matches_reference(golden, tag, g, start):
    r = N.solve(g, start(), None, -1, 1 / 3000, 4.0)
    _check_solve(r, golden[tag], tag)
    assert r["status"] == "converged" and r["steps"] > 3


@pytest.mark.parametrize("fix", [True, False])
def test_restated_environment_matches_reference(golden, fix):
    z = golden["env_fix" if fix else "env_free"]
    np.random.seed(0)
    env = N.Restated(3000, fix)
    keys = [str(k) for k in z["info_keys"]]
    first = {}
    for t in range(6):
        _, _, done, info = env.step(env.gt_control())
        assert done is False
        assert sorted(info) == ([str(k) for k in z["first_info_keys"]] if t == 0 else keys)
        # one rounding of an entry is relative to what it sums (info_scales); a relative entry carries that of both its terms
        scales = {k: max(N.info_scales(env).get(k, 0.0), abs(info[k])) for k in N.INFO_KEYS}
        if t == 0:
            first = {k: (abs(info[k] + 1e-9), scales[k]) for k in N.INFO_KEYS}
        for k, want in zip(keys, z["infos"][t]):
            if k in info:
                base = k.replace("drag_reduction_relative", "drag_reduction")
                allowed = scales[base] if base == k else scales[base] / first[base][0] + abs(want) * first[base][1] / first[base][0]
                assert abs(info[k] - want) <= 4 * N.EPS * allowed, (t, k, info[k], want)
        assert env.F == z["F"][t]
        if fix:
            assert env.fixed[t]["bisections"] == int(z["bisections"][t])
        if t == 0 and not fix:
            f = golden["fixed"]
            r = N.solve_fixed_mass(env.g, (env.p, env.u, env.v), env.gt_control(), np.mean(abs(env.u)), 0, 3 * env.F, env.nu, env.F)
            assert r["result_f"] == float(f["result_f"]) and r["bisections"] == int(f["bisections"]) and r["steps"] == int(f["steps"])
            _close(r["flow"], f["flow"], "fixed-mass flow")
            assert abs(r["error"] - float(f["error"])) <= TOL * float(f["flow"])
    for k in ("p", "u", "v"):
        _close(getattr(env, k), z[k], f"environment {k} after six steps")
    assert sorted(set(keys) - set(str(k) for k in z["first_info_keys"])) == sorted(k.replace("drag_reduction", "drag_reduction_relative") for k in N.INFO_KEYS)


def _plan(text, argv=()):
    import yaml
    from pde_policylearning_amd import run_control as RC
    return RC.plan_from_yaml(RC.build_parser().parse_args(list(argv)), yaml.safe_load(text))


def test_run_plan_from_python_env_yaml():
    plan = _plan(PYTHON_ENV_RNO, ["--ensemble", "8"])
    assert plan.env_name == "NSControlEnv2D" and plan.policies == ["gt", "unmanipulated"] and plan.steps == 301
    assert plan.fix_flow is True and plan.Re == 3000 and plan.detect_plane == -10 and plan.bc_type == "original"
    assert plan.ensemble == 8 and plan.collect_folder is None and not plan.state_path_name
    one = _plan(PYTHON_ENV_RNO.replace("policy_name:\n  - gt\n  - unmanipulated", "policy_name: unmanipulated"))
    assert one.policies == ["unmanipulated"] and one.ensemble == 1
    with pytest.raises(ValueError, match="collect_data is not supported with env_name NSControlEnv2D"):
        _plan(PYTHON_ENV_RNO.replace("collect_data: false", "collect_data: true"))
    with pytest.raises(NotImplementedError):
        _plan(PYTHON_ENV_RNO.replace("  - unmanipulated", "  - rand"))
    with pytest.raises(RuntimeError, match="Not supported policy name"):
        _plan(PYTHON_ENV_RNO.replace("  - unmanipulated", "  - rno"))
    with pytest.raises(RuntimeError, match="Not supported environment"):
        _plan(PYTHON_ENV_RNO.replace("env_name: NSControlEnv2D", "env_name: NSControlEnv1D"))
    # a plan that names the 3-D environment, or none, is what it was: it still asks for its initial condition
    with pytest.raises(ValueError, match="initial condition"):
        _plan(PYTHON_ENV_RNO.replace("env_name: NSControlEnv2D", "env_name: NSControlEnvMatlab").replace(
            "policy_name:\n  - gt\n  - unmanipulated", "policy_name: gt"))


def test_environment_has_no_cpu_path():
    from pde_policylearning_amd.libs.envs.ns_control_2d import NSControlEnv2D
    with pytest.raises(RuntimeError, match="no CPU path"):
        NSControlEnv2D(argparse.Namespace(fix_flow=True, Re=3000), detect_plane=-10, bc_type="original", device="cpu")


def test_long_double_restatement_runs():
    """the floors of the GPU tests come from this second evaluation: it has to be a different precision on this host"""
    assert np.finfo(np.longdouble).eps < N.EPS, "np.longdouble is no wider than float64 on this platform"
    g = N.Grid(9, 12)
    a, b = N.solve(g, N.small_start(), None, 3, 1 / 3000, 4.0), N.solve(g, N.small_start(), None, 3, 1 / 3000, 4.0, dtype=np.longdouble)
    assert b["u"].dtype == np.longdouble and a["steps"] == b["steps"] == 3
    assert 0 < N.rel(a["p"], b["p"]) < 1e-12
