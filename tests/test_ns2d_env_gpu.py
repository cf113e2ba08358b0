"""NSControlEnv2D on the GPU against the numpy restatement of the reference (tests/ns2d_cases.py) and against the values the
reference's own class produced (tests/golden/ns2d_reference.npz).

Tolerance: the project's rule (tests/control_loop_cases.py), bound = min(16 * max(floor, eps), 1e-9); the floor of a compared
field is the max-norm distance between the float64 and the long-double restatement divided by max|field|, measured here on the
CPU at the size at hand.  Step counts, bisection counts and the bisected force are compared exactly; before that, the test
asserts on the CPU that no decision of the restatement sits within rounding of its threshold.  Every distance, floor and bound
goes to profiles/r15_ns2d_errors.txt before anything is asserted."""
import argparse
import functools

import numpy as np
import pytest
import torch

from tests import hygiene as H
from tests import ns2d_cases as N
from tests.control_loop_cases import bits_equal, to_dev, to_np
from tests.judging import dev  # noqa: F401
from tests.util import load_golden

pytestmark = pytest.mark.gpu
EPS = N.EPS
LD = np.longdouble
N_IDX = {"p": 0, "u": 1, "v": 2}


@pytest.fixture(scope="module")
def golden():
    return load_golden("ns2d_reference")


def _stack(dev, states):
    return to_dev(dev, *(np.stack([s[k] for s in states]) for k in range(3)))


def _field_rows(tag, G, A, L):
    """rows for judge(): G the GPU's result, A the float64 restatement, L the long-double one (dicts with p, u, v, bulk_v)"""
    rows = [(f"{tag} {k}", N.rel(G[k], A[k]), N.rel(A[k], L[k]), EPS) for k in ("p", "u", "v")]
    rows.append((f"{tag} bulk_v", abs(float(G["bulk_v"]) - float(A["bulk_v"])) / float(A["bulk_v"]),
                 float(abs(LD(A["bulk_v"]) - L["bulk_v"]) / L["bulk_v"]), EPS))
    return rows


# ---------------------------------------------------------------------------------------------------------------------------
# 1. capped solve, max_step = 3
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ny,nx", N.CAPPED_GRIDS)
def test_capped_solve(dev, golden, ny, nx):
    from pde_policylearning_amd import functional as F
    g = N.Grid(ny, nx)
    states, bcs = N.capped_case(ny, nx)
    p, u, v = _stack(dev, states)
    lo, hi = to_dev(dev, *N.bc_rows(bcs, nx))
    Fs, nus = to_dev(dev, np.array(N.CAPPED_F), np.array(N.CAPPED_NU))
    out = F.ns2d_solve(g.engine(), p, u, v, Fs, nus, lo, hi, max_step=3)
    torch.cuda.synchronize()
    host, rows, steps = to_np(out), [], []
    for b, (st, bc) in enumerate(zip(states, bcs)):
        A = N.solve(g, st, bc, 3, N.CAPPED_NU[b], N.CAPPED_F[b])
        L = N.solve(g, st, bc, 3, N.CAPPED_NU[b], N.CAPPED_F[b], dtype=LD)
        assert A["steps"] == L["steps"]
        G = {"p": to_np(p[b]), "u": to_np(u[b]), "v": to_np(v[b]), "bulk_v": host[b, 0]}
        rows += _field_rows(f"{ny}x{nx} env {b}", G, A, L)
        z = golden[f"capped_{ny}x{nx}_{b}"]
        rows += [(f"{ny}x{nx} env {b} {k} vs the reference", N.rel(G[k], z[k]), N.rel(A[k], L[k]), EPS) for k in ("p", "u", "v")]
        steps.append((int(host[b, 1]), A["steps"], F.NS2D_STATUS[int(host[b, 2])], A["status"]))
    N.judge(f"capped solve {ny}x{nx}", rows)
    for got, want, st_got, st_want in steps:
        assert got == want and st_got == st_want, steps
    # null wall pointers are zero walls: environment 2 alone, without rows, gives the bits of its row in the batch
    p2, u2, v2 = _stack(dev, states[2:])
    out2 = F.ns2d_solve(g.engine(), p2, u2, v2, Fs[2:].clone(), nus[2:].clone(), None, None, max_step=3)
    assert bits_equal(p2[0], p[2]) and bits_equal(u2[0], u[2]) and bits_equal(v2[0], v[2]) and bits_equal(out2[0], out[2])


# ---------------------------------------------------------------------------------------------------------------------------
# 2. converged solve
# ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _converged(tag):
    g, st = (N.Grid(9, 12), N.small_start()) if tag == "conv_9x12" else (N.Grid(41, 41), N.seeded_start())
    hist = []
    A = N.solve(g, st, None, -1, 1 / 3000, 4.0, history=hist)
    L = N.solve(g, st, None, -1, 1 / 3000, 4.0, dtype=LD)
    return g, st, A, L, hist


@pytest.mark.parametrize("tag", ["conv_9x12", "conv_41x41"])
def test_converged_solve(dev, golden, tag):
    from pde_policylearning_amd import functional as F
    g, st, A, L, hist = _converged(tag)
    # CPU precondition: the count cannot hinge on rounding
    margin = min(abs(h - 1e-2) for h in hist)
    assert margin > 1e-6 and A["steps"] == L["steps"] == len(hist) and A["status"] == "converged", (margin, A["steps"], L["steps"])
    p, u, v = _stack(dev, [st])
    un, vn = torch.empty_like(u), torch.empty_like(v)
    out = to_np(F.ns2d_solve(g.engine(), p, u, v, 4.0, 1 / 3000, un=un, vn=vn))
    G = {"p": to_np(p[0]), "u": to_np(u[0]), "v": to_np(v[0]), "bulk_v": out[0, 0]}
    rows = _field_rows(tag, G, A, L)
    rows += [(f"{tag} {k}", N.rel(to_np(t[0]), A[k]), N.rel(A[k], L[k]), EPS) for k, t in (("un", un), ("vn", vn))]
    rows += [(f"{tag} {k} vs the reference", N.rel(G[k], golden[tag][k]), N.rel(A[k], L[k]), EPS) for k in ("p", "u", "v")]
    N.judge(f"converged solve {tag} ({A['steps']} steps, closest udiff to the threshold {margin:.1e})", rows)
    assert int(out[0, 1]) == A["steps"] == int(golden[tag]["steps"]) and F.NS2D_STATUS[int(out[0, 2])] == "converged"


def test_loop_exits(dev):
    from pde_policylearning_amd import functional as F
    g, st, A, _, _ = _converged("conv_9x12")

    def run(force=4.0, **kw):
        t = _stack(dev, [st])
        return t, to_np(F.ns2d_solve(g.engine(), *t, force, 1 / 3000, **kw))
    t0, out0 = run(force=0.0)                                   # udiff < 0 after the first step
    assert N.solve(g, st, None, -1, 1 / 3000, 0.0)["steps"] == 1
    assert int(out0[0, 1]) == 1 and F.NS2D_STATUS[int(out0[0, 2])] == "converged"
    tm, outm = run(max_step=-1)
    t1, out1 = run(max_step=1)                              # `max_step > 1 and ...`: 1 does not cap
    assert int(out1[0, 1]) == A["steps"] and all(bits_equal(a, b) for a, b in zip(t1, tm)) and np.array_equal(out1, outm)
    t2, out2 = run(max_step=2)
    assert int(out2[0, 1]) == 2 and F.NS2D_STATUS[int(out2[0, 2])] == "max_step"
    # update_state=False leaves the state alone and still reports
    p, u, v = _stack(dev, [st])
    keep = [t.clone() for t in (p, u, v)]
    outn = to_np(F.ns2d_solve(g.engine(), p, u, v, 4.0, 1 / 3000, update_state=False))
    assert all(bits_equal(a, b) for a, b in zip((p, u, v), keep)) and np.array_equal(outn, outm)


# ---------------------------------------------------------------------------------------------------------------------------
# 3. the cap
# ---------------------------------------------------------------------------------------------------------------------------
def test_step_cap(dev):
    from pde_policylearning_amd import functional as F
    from pde_policylearning_amd.libs.envs.ns_control_2d import NSControlEnv2D
    g = N.Grid(6, 7)
    states, _ = N.capped_case(6, 7)
    p, u, v = _stack(dev, states[:1])
    keep = [t.clone() for t in (p, u, v)]
    out = F.ns2d_solve(g.engine(), p, u, v, 4.0, 1 / 3000, u_diff_thre=-1.0, step_cap=20)
    torch.cuda.synchronize()                                # the launch returns normally
    out = to_np(out)
    assert int(out[0, 1]) == 21 and F.NS2D_STATUS[int(out[0, 2])] == "cap"
    assert all(bits_equal(a, b) for a, b in zip((p, u, v), keep))      # the reference raises before it stores anything
    assert N.solve(g, states[0], None, -1, 1 / 3000, 4.0, u_diff_thre=-1.0, step_cap=20)["steps"] == 21
    np.random.seed(0)
    env = NSControlEnv2D(argparse.Namespace(fix_flow=False, Re=3000), detect_plane=-10, bc_type="original", device=dev)
    np.random.seed(0)
    ra = N.Restated(3000, False)
    assert N.solve(ra.g, (ra.p, ra.u, ra.v), None, -1, ra.nu, 8.0)["steps"] > 3      # CPU precondition of the second refusal below
    env.step_cap = 2
    with pytest.raises(RuntimeError, match="Not converged solving!"):
        env.solve(None, -1, env.p, env.u, env.v, env.dx, env.dy, env.dt, env.rho, env.nu, env.F, update_state=True, u_diff_thre=-1.0)
    with pytest.raises(RuntimeError, match="Not converged solving!"):
        env.solve_fixed_mass(None, 1.0, 8.0, 12.0, verbose=False)      # the bracket solve at F = 8 needs more than two steps


# ---------------------------------------------------------------------------------------------------------------------------
# 4. fixed mass
# ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _after_one_step():
    np.random.seed(0)
    env = N.Restated(3000, False)
    env.step(env.gt_control())
    bc = env.gt_control()
    target = float(np.mean(abs(env.u)))
    state = (env.p.copy(), env.u.copy(), env.v.copy())
    A = N.solve_fixed_mass(env.g, state, bc, target, 0, 3 * env.F, env.nu, env.F)
    L = N.solve_fixed_mass(env.g, state, bc, target, 0, 3 * env.F, env.nu, env.F, dtype=LD)
    return env, state, bc, target, A, L


def test_fixed_mass(dev, golden):
    from pde_policylearning_amd import functional as F
    env, state, bc, target, A, L = _after_one_step()
    # CPU precondition: no branch of the bisection and no exit test sits within rounding of its threshold
    assert A["status"] == "ok" and A["bisections"] >= 2
    for mid, flow, err in A["trace"]:
        assert abs(flow - target) > 1e-9 and abs(err - 1e-4) > 1e-9, A["trace"]
    assert A["bisections"] == L["bisections"] and float(L["result_f"]) == A["result_f"]
    p, u, v = _stack(dev, [state])
    keep = [t.clone() for t in (p, u, v)]
    lo, hi = to_dev(dev, *N.bc_rows([bc], env.g.nx))
    out = to_np(F.ns2d_fixed_mass(env.g.engine(), p, u, v, env.F, env.nu, target, 0.0, 3 * env.F, lo, hi))[0]
    rows = [("fixed mass flow", abs(out[1] - A["flow"]) / A["flow"], float(abs(LD(A["flow"]) - L["flow"]) / L["flow"]), EPS),
            ("fixed mass error (relative to the flow)", abs(out[2] - A["error"]) / A["flow"], float(abs(LD(A["error"]) - L["error"]) / L["flow"]), EPS)]
    N.judge(f"fixed mass 41x41 ({A['bisections']} bisections)", rows)
    assert out[0] == A["result_f"] == float(golden["fixed"]["result_f"])
    assert int(out[3]) == A["bisections"] == int(golden["fixed"]["bisections"])
    assert int(out[4]) == A["steps"] == int(golden["fixed"]["steps"]) and F.NS2D_FIXED_STATUS[int(out[5])] == "ok"
    assert all(bits_equal(a, b) for a, b in zip((p, u, v), keep))
    for far in (10.0, 0.01):                                # above max_flow, below min_flow: (F, target, 0)
        o = to_np(F.ns2d_fixed_mass(env.g.engine(), p, u, v, env.F, env.nu, far, 0.0, 3 * env.F, lo, hi))[0]
        assert N.solve_fixed_mass(env.g, state, bc, far, 0, 3 * env.F, env.nu, env.F)["status"] == "overflow"
        assert (o[0], o[1], o[2], int(o[3])) == (env.F, far, 0.0, 0) and F.NS2D_FIXED_STATUS[int(o[5])] == "overflow"
    assert all(bits_equal(a, b) for a, b in zip((p, u, v), keep))


# ---------------------------------------------------------------------------------------------------------------------------
# 5. the environment
# ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _restated_rollout(fix, dtype):
    np.random.seed(0)
    env = N.Restated(3000, fix, dtype=dtype)
    recs = []
    for _ in range(6):
        ptop, div, _, info = env.step(env.gt_control())
        recs.append({"ptop": ptop.copy(), "div": div, "info": dict(info), "F": env.F, "state": (env.p.copy(), env.u.copy(), env.v.copy()),
                     "scales": N.info_scales(env)})
    return env, recs


@pytest.mark.parametrize("fix", [True, False])
def test_environment(dev, golden, fix):
    from pde_policylearning_amd.libs.envs.ns_control_2d import NSControlEnv2D
    ra, A = _restated_rollout(fix, np.float64)
    rl, L = _restated_rollout(fix, LD)
    # CPU precondition: both evaluations bisect to the same force, so the long-double run is a floor and not another path
    assert [float(r["F"]) for r in L] == [r["F"] for r in A] and ra.init_steps == rl.init_steps
    if fix:
        for fm in ra.fixed:
            assert all(abs(flow - ra.init_bulk_v) > 1e-9 and abs(err - 1e-4) > 1e-9 for _, flow, err in fm["trace"])
    z = golden["env_fix" if fix else "env_free"]
    zkeys = [str(k) for k in z["info_keys"]]
    np.random.seed(0)
    env = NSControlEnv2D(argparse.Namespace(fix_flow=fix, Re=3000), detect_plane=-10, bc_type="original", device=dev)
    rows, exact = [], []
    first = None
    for t in range(6):
        ptop, div, done, info = env.step(env.gt_control())
        a, l = A[t], L[t]
        assert done is False and sorted(info) == sorted(a["info"]) == ([str(k) for k in z["first_info_keys"]] if t == 0 else zkeys)
        exact.append((env.F, a["F"], float(z["F"][t])))
        for k, f in zip(("p", "u", "v"), (env.p, env.u, env.v)):
            rows.append((f"it {t} {k}", N.rel(to_np(f[0]), a["state"][N_IDX[k]]), N.rel(a["state"][N_IDX[k]], l["state"][N_IDX[k]]), EPS))
        rows.append((f"it {t} pressure_top", N.rel(to_np(ptop), a["ptop"]), N.rel(a["ptop"], l["ptop"]), EPS))
        assert div == info["drag_reduction/4_1_-|divergence|"]
        for k in N.INFO_KEYS:
            want = a["info"][k]
            s = max(a["scales"].get(k, 0.0), abs(want))
            own = abs(want) if want != 0 else 1.0
            rows.append((f"it {t} {k}", abs(info[k] - want) / s, float(abs(LD(want) - l["info"][k]) / s), EPS, abs(info[k] - want) / own))
            ref = float(z["infos"][t][zkeys.index(k)])
            rows.append((f"it {t} {k} vs the reference", abs(info[k] - ref) / s, float(abs(LD(want) - l["info"][k]) / s), EPS))
        if t == 0:
            first = dict(info)
            assert not any(k.startswith("drag_reduction_relative") for k in info)       # the first cal_relative_info is {}
        else:
            for k in N.INFO_KEYS:
                assert info[k.replace("drag_reduction", "drag_reduction_relative")] == info[k] / (first[k] + 1e-9)
    N.judge(f"environment, six steps of gt_control, fix_flow {fix}", rows)
    for got, want, ref in exact:
        assert got == want == ref, exact
    if fix:
        assert int(env.last_fixed[0, 3]) == ra.fixed[-1]["bisections"] == int(z["bisections"][-1])
    for k, f in zip(("p", "u", "v"), (env.p, env.u, env.v)):
        assert N.rel(to_np(f[0]), z[k]) <= N.bound(N.rel(A[-1]["state"][N_IDX[k]], L[-1]["state"][N_IDX[k]]))
    # the surface around step
    p1, p2 = env.get_boundary_pressures()
    assert bits_equal(p1, env.p[0, 0]) and bits_equal(p2, env.get_top_pressure()) and bits_equal(p2, env.p[0, -1])
    state = env.get_state()
    assert "v_scale" not in state and np.array_equal(state["u"], to_np(env.u[0]))
    env.set_state(state)
    assert abs(env.cal_bulk_v() - np.mean(abs(state["u"]))) <= 16 * EPS * np.mean(abs(state["u"]))
    for name, a in (("vis_state", ()), ("plot_spatial_distribution", (0,)), ("cal_dpdx_reverse", ()), ("reward_gt", ()), ("reward_td", (0, 0, 0))):
        with pytest.raises(NotImplementedError):
            getattr(env, name)(*a)



# ---------------------------------------------------------------------------------------------------------------------------
# 6. ensemble
# ---------------------------------------------------------------------------------------------------------------------------
def _ensemble_run(dev, Re, ensemble):
    from pde_policylearning_amd.libs.envs.ns_control_2d import NSControlEnv2D
    np.random.seed(0)
    env = NSControlEnv2D(argparse.Namespace(fix_flow=True, Re=Re), detect_plane=-10, bc_type="original", ensemble=ensemble, device=dev)
    last = None
    for _ in range(3):
        last = env.step(env.gt_control())
    return env, last


def test_ensemble(dev):
    Re = [1000.0, 3000.0, 3000.0, 5000.0]
    env, (ptop, div, done, info) = _ensemble_run(dev, Re, 4)
    assert isinstance(div, list) and len(div) == 4 and isinstance(info, list) and len(info) == 4 and tuple(ptop.shape) == (4, 41)
    fields = lambda e: (e.p, e.u, e.v, e.un, e.vn, e._F)
    for b in (0, 1, 3):
        one, (p1, d1, _, i1) = _ensemble_run(dev, Re[b], 1)
        assert isinstance(i1, dict) and tuple(p1.shape) == (41,)
        for f4, f1 in zip(fields(env), fields(one)):
            assert bits_equal(f4[b], f1[0]), f"environment {b} differs from its own B = 1 run"
        assert bits_equal(ptop[b], p1) and info[b] == i1 and div[b] == d1
    for f in fields(env):
        assert bits_equal(f[1], f[2])
    assert info[1] == info[2] and info[0] != info[1]
    again, (ptop2, div2, _, info2) = _ensemble_run(dev, Re, 4)
    assert all(bits_equal(a, b) for a, b in zip(fields(env), fields(again))) and bits_equal(ptop, ptop2) and info == info2 and div == div2


# ---------------------------------------------------------------------------------------------------------------------------
# 7. routes and operands
# ---------------------------------------------------------------------------------------------------------------------------
def test_launches_and_refusals(dev):
    from pde_policylearning_amd import _lib
    from pde_policylearning_amd import functional as F
    from pde_policylearning_amd.libs.envs.ns_control_2d import NSControlEnv2D
    np.random.seed(0)
    env = NSControlEnv2D(argparse.Namespace(fix_flow=True, Re=[2000.0, 3000.0, 4000.0]), detect_plane=-10, bc_type="original", ensemble=3,
                         device=dev)
    with _lib.launch_log() as log:
        env.step(env.gt_control())
    assert [r["name"] for r in log.records] == ["k_ns2d_solve", "k_ns2d_fixed_mass", "k_ns2d_diag"]
    assert all(r["grid"] == (3, 1, 1) and r["variant"] == r["name"] for r in log.records)      # one workgroup per environment
    assert log.records[0]["lds"] == log.records[1]["lds"] == (7 * 41 * 41 + 128) * 8 and log.records[0]["block"] == (1024, 1, 1)
    env.fix_flow = False
    with _lib.launch_log() as log:
        env.step(0, env.gt_control()[1])                    # step(opV1, opV2)
    assert [r["name"] for r in log.records] == ["k_ns2d_solve", "k_ns2d_diag"]

    g = N.Grid(9, 12)
    p, u, v = _stack(dev, [N.small_start()])
    solve = lambda p=p, u=u, v=v, **kw: F.ns2d_solve(g.engine(), p, u, v, 4.0, 1 / 3000, max_step=3, **kw)
    with pytest.raises(RuntimeError, match=r"`u` must be torch.float64"):
        solve(u=u.float())
    with pytest.raises(RuntimeError, match=r"`v` must live on cuda"):
        solve(v=v.cpu())
    with pytest.raises(RuntimeError, match=r"`p` must live on the GPU"):
        solve(p=p.cpu())
    wide = torch.zeros((1, 9, 24), dtype=torch.float64, device=dev)
    with pytest.raises(RuntimeError, match=r"`u` must be contiguous"):
        solve(u=wide[:, :, ::2])
    with pytest.raises(RuntimeError, match=r"`bc_hi` must have shape \(1, 12\)"):
        solve(bc_hi=torch.zeros((1, 11), dtype=torch.float64, device=dev))
    with pytest.raises(RuntimeError, match=r"`target` must have 1 elements"):
        F.ns2d_fixed_mass(g.engine(), p, u, v, 4.0, 1 / 3000, torch.zeros(2, dtype=torch.float64, device=dev), 0.0, 12.0)
    with pytest.raises(RuntimeError, match=r"`nu` must be torch.float64"):
        F.ns2d_diagnostics(N.Grid(41, 41).engine(), *_stack(dev, [N.seeded_start()]), torch.ones(1, device=dev))
    # beyond the carve: 54 x 54 = 2916 points > 2907
    big = N.Grid(54, 54)
    z = torch.zeros((1, 54, 54), dtype=torch.float64, device=dev)
    with pytest.raises(RuntimeError, match=r"code -2.*exceeds 2907 points"):
        F.ns2d_solve(big.engine(), z, z.clone(), z.clone(), 4.0, 1 / 3000)
    with pytest.raises(RuntimeError, match=r"code -2.*at least 3"):
        F.ns2d_solve(N.Grid(2, 12).engine(), z[:, :2, :12].contiguous(), z[:, :2, :12].contiguous(), z[:, :2, :12].contiguous(), 4.0, 1 / 3000)
    with pytest.raises(RuntimeError, match=r"code -2.*at least 11"):
        F.ns2d_diagnostics(g.engine(), p, u, v, 1 / 3000)
    ok = torch.zeros((1, 53, 54), dtype=torch.float64, device=dev)      # 2862 points: the largest tested grid that fits
    out = to_np(F.ns2d_solve(N.Grid(53, 54).engine(), ok, ok.clone(), ok.clone(), 4.0, 1 / 3000, max_step=2))
    assert int(out[0, 1]) == 2


def test_run_control_runs_the_listed_policies(dev, capsys):
    """run_ns2d on the plan of the python_env_rno.yaml fixture, shortened: both policies from the same start state"""
    import yaml
    from pde_policylearning_amd import run_control as RC
    from tests.util import GOLDEN
    import os
    cfg = yaml.safe_load(open(os.path.join(GOLDEN, "python_env_rno.yaml")))
    cfg["control_timestep"] = 2
    plan = RC.plan_from_yaml(RC.build_parser().parse_args(["--ensemble", "2"]), cfg)
    res = RC.run(plan)
    assert list(res) == ["gt", "unmanipulated"]
    for r in res.values():
        assert r.log.shape == (3, 2, 7) and len(r.infos) == 3 and len(r.infos[0]) == 2 and r.exploded_at is None
        assert np.isfinite(r.log).all() and np.array_equal(r.log[:, 0], r.log[:, 1])       # one start state, one Re
        assert not any(k.startswith("drag_reduction_relative") for k in r.infos[0][0]) and len(r.infos[1][0]) == 14
    gt, un = res["gt"].log, res["unmanipulated"].log
    assert not np.array_equal(gt[0], un[0])                   # the same start, another wall condition
    # gt holds the flow of its first step by bisection; unmanipulated takes its target before the first step (reset_init),
    # finds it below the bracket and keeps F = 4 (solve_fixed_mass returns self.F)
    assert gt[0, 0, 4] != 4.0 and (un[:, :, 4] == 4.0).all()
    np.random.seed(plan.seed)
    ra = N.Restated(3000, True)
    first = ra.step(ra.gt_control())[3]
    assert gt[0, 0, 4] == first["drag_reduction/3_2_dPdx_required"]
    out = capsys.readouterr().out
    assert "gt env 1 (iteration 2)" in out and "unmanipulated env 0 (iteration 2)" in out
    one = RC.run(RC.plan_from_yaml(RC.build_parser().parse_args([]), dict(cfg, policy_name="gt", control_timestep=1)))
    assert one.log.shape == (2, 1, 7) and isinstance(one.infos[0], dict) and np.array_equal(one.log[:, 0], gt[:2, 0])
    # an exploding policy ends its own rollout and the next one still runs
    old = RC.EXPLODE_AT
    RC.EXPLODE_AT = 0.0
    try:
        res = RC.run(plan)
    finally:
        RC.EXPLODE_AT = old
    assert [r.exploded_at for r in res.values()] == [0, 0] and all(r.log.shape == (1, 2, 7) for r in res.values())
    assert "Control exploded! policy unmanipulated, iteration 0" in capsys.readouterr().out


@pytest.mark.parametrize("ny,nx,B", [(6, 7, 2), (41, 41, 3)])
def test_hygiene(dev, ny, nx, B):
    """one solve, one fixed-mass launch and the diagnostics through the poisoned-buffer harness: outputs bitwise equal under
    every pattern, guard bands intact, read-only inputs unchanged.  Nothing in these buffers is turned into an address."""
    from pde_policylearning_amd import functional as F
    g = N.Grid(ny, nx)
    rng = np.random.default_rng(ny)
    states = [N.small_start(ny, nx, seed=s) for s in range(B)]
    p, u, v = _stack(dev, states)
    lo, hi = to_dev(dev, 0.02 * rng.standard_normal((B, nx)), 0.02 * rng.standard_normal((B, nx)))
    inputs = {"p": p, "u": u, "v": v, "lo": lo, "hi": hi, "F": torch.full((B,), 4.0, dtype=torch.float64, device=dev),
              "nu": torch.full((B,), 1 / 3000, dtype=torch.float64, device=dev)}

    def fn(inp, after_forward):
        un, vn = H.guarded(torch.empty_like(inp["u"])), H.guarded(torch.empty_like(inp["v"]))      # outputs inside guard bands
        res = {"fixed": F.ns2d_fixed_mass(g.engine(), inp["p"], inp["u"], inp["v"], inp["F"], inp["nu"], 1.0, 0.0, 12.0, inp["lo"], inp["hi"]),
               "report": F.ns2d_solve(g.engine(), inp["p"], inp["u"], inp["v"], inp["F"], inp["nu"], inp["lo"], inp["hi"], max_step=3,
                                      update_state=False)}
        if ny >= 11:
            res["diag"], res["ptop"] = F.ns2d_diagnostics(g.engine(), inp["p"], inp["u"], inp["v"], inp["nu"], dpdx=inp["F"])
        after_forward()
        P, U, V = inp["p"].clone(), inp["u"].clone(), inp["v"].clone()
        res["solve"] = F.ns2d_solve(g.engine(), P, U, V, inp["F"], inp["nu"], inp["lo"], inp["hi"], max_step=3, un=un, vn=vn)
        res.update({"P": P, "U": U, "V": V, "un": un, "vn": vn})
        return res
    H.assert_clean(f"ns2d hygiene {ny}x{nx} B={B}", fn, inputs)
