"""Channel-flow environment step on the GPU against the float64 restatement of tests/chanflow_step_reference.py.

Tolerances (the float64 floor rule, tests/judging.py).  Nothing here is tuned to what the kernels give.  For every compared
quantity the test first measures, on the CPU and at the size at hand, the FLOOR: the distance between the restatement solved by dense numpy.linalg.solve and the same
restatement solved by a float64 Thomas recurrence.  The GPU gets 16 x that floor (its transforms sum in another order and
contract to FMA), never more than 1e-9 = cond * eps of the worst Poisson system (7e6 x 1.1e-16).  Two remarks on the floor:
  - a floor cannot be below the resolution of the number format: two float64 evaluations of one quantity differ by eps =
    2.2e-16 relative unless they are bitwise equal, and the two CPU arms sometimes are (a scalar such as dPdx came out with a
    distance of exactly 0 at the small sizes).  The floor used is max(measured distance, resolution), resolution = eps.
  - quantities that are differences of nearly equal numbers are measured against the scale of what is subtracted, because
    that is what one rounding is relative to:  dPdx_new = (dPdx + 2 (meanU0 - meanU) / dt) / 2 carries the rounding of a bulk
    velocity divided by dt, so its resolution is eps * |meanU0| / dt / |dPdx|;  sum(div) after a projection is a sum of
    rounding residues, measured against the sum of |du/dx| + |dv/dy| + |dw/dz|;  the wall shear stress and the pressure
    mean are means of signed terms, measured against the mean of their absolute values.
Every measured value goes to profiles/r11_chanflow_step_errors.txt: floor, resolution, bound and GPU distance, beside them the
bound of the plain rule (16 x the measured floor, cap 1e-9, no resolution) and, for the entries measured against a scale, the
raw errors relative to the entry's own magnitude - so that what the two remarks loosen stays visible."""
import functools
import os

import numpy as np
import pytest
import torch

from tests import chanflow_step_reference as R
from tests import control_loop_cases as K
from tests.judging import CAP64, EPS64, SectionLog, dev, judge_floor  # noqa: F401

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOG = SectionLog(os.path.join(ROOT, "profiles", "r11_chanflow_step_errors.txt"))
DT = K.DT
_log = LOG.replace
# rows: (name, gpu distance, floor, resolution[, (raw gpu, raw floor)]), with the plain rule's bound beside each (module docstring)
_judge = functools.partial(judge_floor, LOG, width=46, plain_rule=True)


def _F():
    from pde_policylearning_amd import functional as F
    return F


# ---------------------------------------------------------------------------------------------------------------------------
# 1, 2: projection
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag,B", [("small", 1), ("odd", 1), ("shipped", 1), ("shipped", 3)])
def test_projection_parity_and_property(dev, tag, B):
    """chanflow_project vs the restatement, relative L2 per field, and the projection property: off each y-plane's xz-mean the
    discrete divergence is at most 1e-10 of the largest divergence entry before (every wavenumber pair but (0,0) is solved
    exactly; (0,0) is singular-regularised).  The restatement itself is held to the same property first."""
    F = _F()
    states = [K.fixture_state(tag, b) for b in range(B)]
    g = states[0][0]
    grid, poisson = K.engine(g)
    U, V, W = K.to_dev(dev, *[np.stack([s[k] for s in states]) for k in (1, 2, 3)])
    F.chanflow_project(grid, poisson, U, V, W)
    got = [K.to_np(t) for t in (U, V, W)]
    rows, prop = [], []
    for b, (_, U0, V0, W0) in enumerate(states):
        dense, thomas = R.project(g, U0, V0, W0), R.project(g, U0, V0, W0, "thomas")
        for n, k in (("U", 0), ("V", 1), ("W", 2)):
            rows.append((f"{n}[{b}]", R.rel(got[k][b], dense[k]), R.rel(thomas[k], dense[k]), EPS64))
        rows.append((f"p_hat[{b}] (floor only)", 0.0, R.rel(thomas[3], dense[3]), EPS64))
        before = np.abs(R.divergence(g, U0, V0, W0)).max()
        off = lambda X: np.abs((lambda d: d - d.mean(axis=(0, 2), keepdims=True))(R.divergence(g, *X))).max() / before
        prop.append((b, off(dense[:3]), off([got[0][b], got[1][b], got[2][b]])))
    lines = []
    for b, ref, gpu in prop:
        lim = 1e-10 if ref <= 1e-10 else 16 * ref
        lines.append(f"sample {b}: off-mean divergence / max |div before|   restatement {ref:.3e}   gpu {gpu:.3e}   bound {lim:.3e}")
        print(lines[-1])
    _log(f"projection property {tag} B={B}", lines)
    _judge(f"projection parity {tag} B={B}", rows)
    for b, ref, gpu in prop:
        assert gpu <= (1e-10 if ref <= 1e-10 else 16 * ref), (b, ref, gpu)


# ---------------------------------------------------------------------------------------------------------------------------
# 3: one RK3 step
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["small", "odd", "shipped"])
@pytest.mark.parametrize("control", ["opposition", "opV1_zero"])
def test_rk3_step(dev, tag, control):
    F = _F()
    g, U0, V0, W0 = K.fixture_state(tag)
    grid, poisson = K.engine(g)
    v1, v2 = R.gt_control(V0, min(10, g.Ny // 3))
    if control == "opV1_zero":
        v1 = np.zeros_like(v1)
    m0 = R.bulk_velocity(g, U0) * 1.001              # so that the pressure-gradient update has something to hold
    dense = R.rk3_step(g, U0, V0, W0, v1, v2, R.DPDX0, m0, DT)
    thomas = R.rk3_step(g, U0, V0, W0, v1, v2, R.DPDX0, m0, DT, "thomas")
    U, V, W, a1, a2 = K.to_dev(dev, U0[None], V0[None], W0[None], v1[None], v2[None])
    dp = torch.full((1,), R.DPDX0, dtype=torch.float64, device=dev)
    mu = torch.full((1,), m0, dtype=torch.float64, device=dev)
    F.chanflow_rk3_step(grid, poisson, U, V, W, a1, a2, dp, mu, DT)
    got = [K.to_np(U)[0], K.to_np(V)[0], K.to_np(W)[0], K.to_np(dp)[0]]
    rows = [(n, R.rel(got[k], dense[k]), R.rel(thomas[k], dense[k]), EPS64) for k, n in enumerate("UVW")]
    rows.append(("dPdx", R.rel(got[3], dense[3]), R.rel(thomas[3], dense[3]), K.dpdx_resolution(m0, dense[3])))
    assert np.array_equal(got[1][:, 0], v1) and np.array_equal(got[1][:, -1], v2)       # the wall condition holds exactly
    _judge(f"rk3 step {tag} {control}", rows)


# ---------------------------------------------------------------------------------------------------------------------------
# 4: closed-loop rollout
# ---------------------------------------------------------------------------------------------------------------------------
def test_rollout_small(dev):
    """20 steps under opposition control.  The floor is the restatement's own sensitivity: a second CPU run whose initial
    state carries a relative 1e-16 seeded perturbation.  At every step the GPU state (U, V, W as one vector) stays within
    16 x the distance between the two CPU runs."""
    F = _F()
    g, U0, V0, W0 = K.fixture_state("small")
    grid, poisson = K.engine(g)
    plane, steps = 3, 20
    m0 = R.bulk_velocity(g, U0)
    rng = np.random.default_rng(11)
    cpu = [(U0, V0, W0, R.DPDX0), tuple(a * (1 + 1e-16 * rng.standard_normal(a.shape)) for a in (U0, V0, W0)) + (R.DPDX0,)]
    U, V, W = K.to_dev(dev, U0[None], V0[None], W0[None])
    dp = torch.full((1,), R.DPDX0, dtype=torch.float64, device=dev)
    mu = torch.full((1,), m0, dtype=torch.float64, device=dev)
    cat = lambda s: np.concatenate([np.asarray(a).ravel() for a in s[:3]])
    lines, bad = [], []
    for it in range(steps):
        cpu = [R.rk3_step(g, *s[:3], *R.gt_control(s[1], plane), s[3], m0, DT) for s in cpu]
        F.chanflow_rk3_step(grid, poisson, U, V, W, -V[:, :, plane, :], -V[:, :, -plane, :], dp, mu, DT)
        floor = R.rel(cat(cpu[1]), cat(cpu[0]))
        got = R.rel(cat([K.to_np(U)[0], K.to_np(V)[0], K.to_np(W)[0]]), cat(cpu[0]))
        ok = got <= min(16 * floor, CAP64)
        lines.append(f"step {it + 1:2d}   cpu perturbed vs cpu {floor:.3e}   gpu vs cpu {got:.3e}   bound {min(16 * floor, CAP64):.3e}   {'ok' if ok else 'MISS'}")
        print(lines[-1])
        if not ok:
            bad.append(lines[-1])
    _log("rollout small, 20 steps, opposition control", lines)
    assert not bad, "\n".join(bad)


# ---------------------------------------------------------------------------------------------------------------------------
# 5: wall pressure, diagnostics, the environment's step
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["small", "odd", "shipped"])
def test_wall_pressure_and_step_info(dev, tag):
    """p1, p2, the full P of cal_pressure and every `info` key of ChannelFlowEnv.step against the restatement"""
    from pde_policylearning_amd.libs.envs.control_env import ChannelFlowEnv
    g, U0, V0, W0 = K.fixture_state(tag)
    env = ChannelFlowEnv(g.Nx, g.Nz, g.dx, g.dz, g.y, g.ym, U0, V0, W0, dt=DT, detect_plane=min(10, g.Ny // 3), device=dev)
    m0 = R.bulk_velocity(g, U0)
    rows = [("meanU0", abs(float(env.meanU0[0]) - m0) / abs(m0), 0.0, EPS64)]
    dense, thomas = R.pressure(g, U0, V0, W0, R.DPDX0), R.pressure(g, U0, V0, W0, R.DPDX0, "thomas")
    p1, p2 = env.get_boundary_pressures()
    P = env.cal_pressure()
    assert tuple(P.shape) == (g.Nx, g.Ny - 1, g.Nz)
    for n, t, k in (("p1", p1, 0), ("p2", p2, 1), ("P", P, 2)):
        rows.append((n, R.rel(K.to_np(t), dense[k]), R.rel(thomas[k], dense[k]), EPS64))
    v1, v2 = env.gt_control()
    w1, w2 = R.gt_control(V0, env.detect_plane)
    assert np.array_equal(K.to_np(v1), w1) and np.array_equal(K.to_np(v2), w2)
    p2g, div, done, info = env.step(v1, v2)
    assert done is False and div == info["drag_reduction/4_1_-|divergence|"]
    ref = {}
    for name, solver in (("dense", "dense"), ("thomas", "thomas")):
        U, V, W, dp = R.rk3_step(g, U0, V0, W0, w1, w2, R.DPDX0, m0, DT, solver)
        p2r = R.pressure(g, U, V, W, dp, solver)[1]
        ref[name] = (R.step_info(g, U, V, W, p2r, dp), p2r, (U, V, W))
    rows.append(("step p2", R.rel(K.to_np(p2g), ref["dense"][1]), R.rel(ref["thomas"][1], ref["dense"][1]), EPS64))
    scales = K.info_scales(g, *ref["dense"][2], ref["dense"][1])
    assert set(R.INFO_KEYS) <= set(info)
    for k in R.INFO_KEYS:
        want, alt = ref["dense"][0][k], ref["thomas"][0][k]
        s = scales.get(k, abs(want))
        res = K.dpdx_resolution(m0, want) if k.endswith("dPdx_reverse_cal") else EPS64
        own = abs(want) if want != 0 else 1.0
        rows.append((k, abs(info[k] - want) / s, abs(alt - want) / s, res, (abs(info[k] - want) / own, abs(alt - want) / own)))
    rel_keys = [k for k in info if k.startswith("drag_reduction_relative")]
    assert len(rel_keys) == len(R.INFO_KEYS) - 1 and all(np.isfinite(info[k]) for k in rel_keys)
    _judge(f"wall pressure and info {tag}", rows)


def test_env_graph_mode_and_state_files(dev, tmp_path):
    """ChannelFlowEnv(graph=True) steps bit for bit like the eager environment (state, dPdx, observation, info), its returned
    p2 survives the next step, dump_state / load_state round-trip through the environment and the graph is rebuilt after
    load_state; the host view of dPdx follows the device value."""
    from pde_policylearning_amd.libs.envs.control_env import ChannelFlowEnv
    g, U0, V0, W0 = K.fixture_state("small")
    mk = lambda graph: ChannelFlowEnv(g.Nx, g.Nz, g.dx, g.dz, g.y, g.ym, U0, V0, W0, dt=DT, detect_plane=3, device=dev, graph=graph)
    eager, graphed = mk(False), mk(True)
    assert eager.dPdx == R.DPDX0
    kept = []
    for it in range(3):
        outs = []
        for env in (eager, graphed):
            p2, div, done, info = env.step(*env.gt_control())
            outs.append((p2, info))
        assert K.bits_equal(outs[0][0], outs[1][0]) and outs[0][1] == outs[1][1], f"step {it}"
        kept.append((outs[1][0], outs[1][0].clone()))
        for n in ("U", "V", "W", "dPdx_dev"):
            assert K.bits_equal(getattr(eager, n), getattr(graphed, n)), n
    assert all(K.bits_equal(a, b) for a, b in kept), "a returned p2 was overwritten by a later step"
    assert eager.dPdx == float(eager.dPdx_dev[0]) != R.DPDX0
    Fu = eager.compute_rhs_py(eager.U[0], eager.V[0], eager.W[0])[0]
    assert K.bits_equal(Fu, eager.compute_rhs_py(eager.U[0], eager.V[0], eager.W[0], eager.dPdx)[0])
    path = str(tmp_path / "state.mat")
    eager.dump_state(path)
    for env in (eager, graphed):
        before = [t.clone() for t in (eager.U, eager.V, eager.W)]
        env.load_state(path)
        for a, n in zip(before, "UVW"):
            assert K.bits_equal(a, getattr(env, n)), n
    graphed.dPdx_dev.copy_(eager.dPdx_dev)
    pe, pg = eager.step(*eager.gt_control())[0], graphed.step(*graphed.gt_control())[0]
    assert K.bits_equal(pe, pg) and K.bits_equal(eager.U, graphed.U)
    z = ChannelFlowEnv(g.Nx, g.Nz, g.dx, g.dz, g.y, g.ym, U0, V0 * 0, W0, dt=DT, detect_plane=3, device=dev)
    z.V_gt.zero_()
    assert np.isfinite(z.reward_gt())                    # a zero reference field costs 0, not nan


# ---------------------------------------------------------------------------------------------------------------------------
# 6: batch, graph, repeatability
# ---------------------------------------------------------------------------------------------------------------------------
def test_batch_graph_and_repeatability_are_bitwise(dev):
    F = _F()
    states = [K.fixture_state("shipped", b) for b in range(3)]
    g = states[0][0]
    grid, poisson = K.engine(g)
    plane = 10

    def run(idx, steps, graphed=False):
        U, V, W = K.to_dev(dev, *[np.stack([states[b][k] for b in idx]) for k in (1, 2, 3)])
        dp = torch.full((len(idx),), R.DPDX0, dtype=torch.float64, device=dev)
        mu = torch.tensor([R.bulk_velocity(g, states[b][1]) for b in idx], dtype=torch.float64, device=dev)
        if graphed:
            gs = F.GraphedChannelStep(grid, poisson, U, V, W, dp, mu, DT)
            for _ in range(steps):
                gs.opV1.copy_(-gs.V[:, :, plane, :])
                gs.opV2.copy_(-gs.V[:, :, -plane, :])
                p1, p2 = gs.step()
            return [t.clone() for t in (gs.U, gs.V, gs.W, gs.dPdx, p1, p2)]
        for _ in range(steps):
            F.chanflow_rk3_step(grid, poisson, U, V, W, -V[:, :, plane, :], -V[:, :, -plane, :], dp, mu, DT)
            p1, p2 = F.chanflow_wall_pressure(grid, poisson, U, V, W, dp)
        return [U, V, W, dp, p1, p2]

    whole = run([0, 1, 2], 2)
    for b in range(3):
        for a, w in zip(run([b], 2), whole):
            assert K.bits_equal(a[0], w[b]), f"sample {b} of a batch differs from the single run"
    eager, again, graph = run([0], 10), run([0], 10), run([0], 10, graphed=True)
    for a, b, c in zip(eager, again, graph):
        assert K.bits_equal(a, b), "two runs from one state differ"
        assert K.bits_equal(a, c), "graph replay differs from eager"
    assert all(torch.isfinite(t).all() for t in eager)


# ---------------------------------------------------------------------------------------------------------------------------
# 8: refusals, and every supported power of two
# ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing(dev):
    F = _F()
    from pde_policylearning_amd import _lib
    g, U0, V0, W0 = K.fixture_state("small")
    grid, poisson = K.engine(g)
    U, V, W = K.to_dev(dev, U0[None], V0[None], W0[None])
    keep = [t.clone() for t in (U, V, W)]
    lib = _lib.lib()
    lib.fno_profile_reset()
    lib.fno_profile_enable(1)
    try:
        with pytest.raises(RuntimeError, match="2..128"):
            big = F.ChannelGrid(256, g.Nz, g.dx, g.dz, g.y, g.ym, g.yg, g.nu)
            F.ChannelPoisson(big)
        with pytest.raises(RuntimeError, match="float64 only"):
            F.chanflow_project(grid, poisson, U.float(), V.float(), W.float())
        with pytest.raises(RuntimeError, match="contiguous"):
            F.chanflow_project(grid, poisson, U.transpose(1, 3).contiguous().transpose(1, 3), V, W)
        with pytest.raises(RuntimeError, match="workspace too small"):
            F.chanflow_project(grid, poisson, U, V, W, ws=torch.empty(4096, dtype=torch.uint8, device=dev))
        g2 = R.Grid(g.Nx + 2, g.Ny, g.Nz)
        wrong = F.ChannelPoisson(F.ChannelGrid(g2.Nx, g2.Nz, g2.dx, g2.dz, g2.y, g2.ym, g2.yg, g2.nu))
        with pytest.raises(RuntimeError, match="does not belong to this grid"):
            F.chanflow_project(grid, wrong, U, V, W)
        with pytest.raises(RuntimeError, match="shape"):
            F.chanflow_rk3_step(grid, poisson, U, V, W, U[:, :, 0, :1], U[:, :, 0, :], torch.zeros(1, dtype=torch.float64, device=dev), 1.0, DT)
        torch.cuda.synchronize()
        assert _lib.profile_summary() == [], "a refused call launched a kernel"
    finally:
        lib.fno_profile_enable(0)
        lib.fno_profile_reset()
    for a, b in zip(keep, (U, V, W)):
        assert torch.equal(a, b)


@pytest.mark.parametrize("N", [8, 16, 64, 128])
def test_every_power_of_two_projects(dev, N):
    """Nx = Nz = N (32 is the shipped grid above) on a short channel: parity with the restatement under the rule of (1)"""
    F = _F()
    g = R.Grid(N, 6, N)
    U0, V0, W0 = R.analytic_state(g, N, noise=0.2)
    grid, poisson = K.engine(g)
    U, V, W = K.to_dev(dev, U0[None], V0[None], W0[None])
    F.chanflow_project(grid, poisson, U, V, W)
    dense, thomas = R.project(g, U0, V0, W0), R.project(g, U0, V0, W0, "thomas")
    _judge(f"projection parity {N} x 6 x {N}",
           [(n, R.rel(K.to_np(t)[0], dense[k]), R.rel(thomas[k], dense[k]), EPS64) for k, (n, t) in enumerate(zip("UVW", (U, V, W)))])
