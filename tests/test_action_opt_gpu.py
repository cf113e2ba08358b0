"""The optimal-observer policy on the GPU (csrc/k_action_opt.h, functional.ctrl_action_*, control.OptimalObserverPolicy):
the four kernels piece by piece, the lifting's input gradient, the observer's input gradient through the engine front, the
whole policy on ControlLoop against the float64 restatement, graph against eager, and the ensemble dimension.  The rule, the
fixture and both restatements live in tests/action_opt_cases.py; every figure goes to profiles/r16_action_opt_errors.txt
before it is asserted."""
import math

import numpy as np
import pytest
import torch

from tests import action_opt_cases as A
from tests import chanflow_step_reference as R
from tests import control_loop_cases as K
from tests.judging import EPS64, dev, judge_floor  # noqa: F401

pytestmark = pytest.mark.gpu


def _plane_stats(plane, seed=3):
    """1-D float64 statistics of `plane` points, drawn as A.stats"""
    g = torch.Generator().manual_seed(seed + plane)
    return 0.05 * torch.randn(plane, generator=g, dtype=torch.float64), 0.2 + 0.1 * torch.rand(plane, generator=g, dtype=torch.float64)


def _objective_inputs(B, P, plane, seed=11):
    g = torch.Generator().manual_seed(seed + 7 * B + 3 * P + plane)
    y = torch.randn(B, P, plane, generator=g)
    a = 0.3 * torch.randn(B, plane, generator=g)
    return y, a


# ---------------------------------------------------------------------------------------------------------------------------
# 1: the objective
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plane", [1024, 1020, 257, 1])
@pytest.mark.parametrize("P", [1, 3])
@pytest.mark.parametrize("B", [1, 3])
def test_objective(dev, B, P, plane):
    """parts against numpy float64 under control_loop_cases.bound(floor), the floor from a second summation order (math.fsum
    against numpy's pairwise sum); dy within one float32 ulp of float32(the float64 value); an all-zero field; environment b
    of the batch bit-equal to its own B = 1 run; two runs bit-equal.  1020, 257 and 1: partial trips and partial workgroups."""
    from pde_policylearning_amd import functional as F
    reg = 0.1
    y, a = _objective_inputs(B, P, plane)
    mean, std = _plane_stats(plane)
    yd, ad, md, sd = y.to(dev), a.to(dev), mean.to(dev), std.to(dev)
    parts, dy = F.ctrl_action_objective(yd, ad, md, sd, A.EPS, reg=reg)
    parts2, dy2 = F.ctrl_action_objective(yd, ad, md, sd, A.EPS, reg=reg)
    assert K.bits_equal(parts, parts2) and K.bits_equal(dy, dy2), "two runs differ"
    S = (std + A.EPS).numpy()
    field = y.double().numpy() * S + mean.numpy()
    a64 = a.double().numpy()
    lines, bad = [], []
    for b in range(B):
        sq, sa = (field[b] ** 2).ravel(), (a64[b] ** 2).ravel()
        nf, na = math.sqrt(np.sum(sq)), math.sqrt(np.sum(sa))
        nf2, na2 = math.sqrt(math.fsum(sq)), math.sqrt(math.fsum(sa))
        want = (nf + reg * na, nf, na)
        other = (nf2 + reg * na2, nf2, na2)
        got = parts[b].cpu().numpy()
        for k, name in enumerate(F.ACTION_PARTS):
            dist, floor = abs(got[k] - want[k]) / abs(want[k]), abs(other[k] - want[k]) / abs(want[k])
            lim = K.bound(floor)
            lines.append(f"[{b}] {name:12s} gpu {dist:.3e}   floor {floor:.3e}   bound {lim:.3e}   {'ok' if dist <= lim else 'MISS'}")
            if not dist <= lim:
                bad.append(lines[-1])
        want_dy = (field[b] / nf * S).astype(np.float32)
        ulps = np.abs(dy[b].cpu().numpy().astype(np.float64) - want_dy.astype(np.float64)) / np.spacing(np.abs(want_dy)).astype(np.float64)
        lines.append(f"[{b}] dy           worst distance from float32(float64 value): {ulps.max():.2f} ulp")
        if not ulps.max() <= 1.0:
            bad.append(lines[-1])
        one_p, one_dy = F.ctrl_action_objective(yd[b:b + 1].contiguous(), ad[b:b + 1].contiguous(), md, sd, A.EPS, reg=reg)
        assert K.bits_equal(one_p[0], parts[b]) and K.bits_equal(one_dy[0], dy[b]), f"environment {b} depends on its batch position"
    A.log_block(f"objective B={B} P={P} plane={plane}", lines)
    assert not bad, "\n".join(bad)
    zp, zdy = F.ctrl_action_objective(torch.zeros_like(yd), ad, torch.zeros_like(md), sd, A.EPS, reg=reg)
    assert not zdy.any() and bool(torch.isfinite(zp).all()) and not zp[:, 1].any()
    assert torch.equal(zp[:, 0], reg * zp[:, 2])


# ---------------------------------------------------------------------------------------------------------------------------
# 2: the update
# ---------------------------------------------------------------------------------------------------------------------------
def _update_reference(dx, a0, S, reg, steps, ref32):
    """torch.optim.Adam on g = dx / S + reg a / |a| per environment; ref32: the reference's two float32 contributions on a
    float32 leaf; else float64.  -> per step {"p", "exp_avg", "exp_avg_sq"} in float64"""
    dt = torch.float32 if ref32 else torch.float64
    p = torch.nn.Parameter(a0.to(dt).clone())
    opt = torch.optim.Adam([p], lr=A.LR, betas=A.BETAS, eps=A.ADAM_EPS)
    out = []
    for t in range(steps):
        with torch.no_grad():
            na = p.norm(dim=1, keepdim=True)
            second = torch.where(na > 0, reg * p / na, torch.zeros_like(p))
            p.grad = ((dx[t].double() / S).to(dt) + second) if ref32 else (dx[t].double() / S + second)
        opt.step()
        st = opt.state[p]
        out.append({"p": p.detach().double().clone(), "exp_avg": st["exp_avg"].double().clone(), "exp_avg_sq": st["exp_avg_sq"].double().clone()})
    return out


@pytest.mark.parametrize("strided", [False, True])
@pytest.mark.parametrize("plane", [1024, 257])
def test_update(dev, plane, strided):
    """steps 1..3 against the float64 formula under the rule (no floor); NaN-filled moments before step 1 are not read; x is
    bit-equal to float32((float64(a_new) - mean) / S) formed by torch from the kernel's own a_new; na == 0 gives a finite g;
    with a strided x the other channels are left alone"""
    from pde_policylearning_amd import functional as F
    B, reg, steps = 2, 0.1, 3
    g = torch.Generator().manual_seed(17 + plane)
    dx = 1e-3 * torch.randn(steps, B, plane, generator=g)
    a0 = 0.3 * torch.randn(B, plane, generator=g)
    mean, std = _plane_stats(plane)
    S = std + A.EPS
    md, sd = mean.to(dev), std.to(dev)
    a = a0.to(dev)
    m = torch.full((B, plane), float("nan"), device=dev)
    v = torch.full((B, plane), float("nan"), device=dev)
    stride = 3 * plane if strided else plane
    x = torch.full((B, 3, plane) if strided else (B, plane), -7.0, device=dev)
    ref64, ref32 = _update_reference(dx, a0, S, reg, steps, False), _update_reference(dx, a0, S, reg, steps, True)
    rows = []
    for t in range(steps):
        parts = torch.zeros(B, 3, dtype=torch.float64, device=dev)
        parts[:, 2] = a.double().norm(dim=1)
        F.ctrl_action_update(dx[t].to(dev), parts, md, sd, A.EPS, a, m, v, x, t + 1, reg=reg, batch_stride=stride)
        got = {"p": a, "exp_avg": m, "exp_avg_sq": v}
        assert all(bool(torch.isfinite(q).all()) for q in got.values()), f"step {t + 1}: not finite"
        for k in got:
            rows.append((f"step {t + 1} {k}", A.rel_err(got[k], ref64[t][k]), A.rel_err(ref32[t][k], ref64[t][k]), 0.0))
        want_x = ((a.double() - md) / (sd + A.EPS)).float()
        assert K.bits_equal(x[:, 0] if strided else x, want_x), f"step {t + 1}: x is not the one rounding of the encoded action"
        if strided:
            assert bool((x[:, 1:] == -7.0).all()), "the update wrote outside channel 0"
    A.judge(f"update plane={plane} strided={strided}", rows)
    # na == 0: the regulariser's term is dropped, g = dx / S stays finite
    a1, m1, v1 = a0.to(dev), torch.zeros(B, plane, device=dev), torch.zeros(B, plane, device=dev)
    F.ctrl_action_update(dx[0].to(dev), torch.zeros(B, 3, dtype=torch.float64, device=dev), md, sd, A.EPS, a1, m1, v1, x, 1, reg=reg,
                         batch_stride=stride)
    g0 = (dx[0].double() / S).float()
    assert bool(torch.isfinite(a1).all()) and torch.equal(m1.cpu(), g0 * torch.tensor(1.0 - A.BETAS[0], dtype=torch.float32))


# ---------------------------------------------------------------------------------------------------------------------------
# 3: begin and finish
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plane", [1024, 1020, 257, 1])
def test_begin_and_finish_bit_for_bit(dev, plane):
    """begin: a = float32(opV2_0) and x = float32((float64(a) - mean) / S), one rounding each, dense and strided; finish:
    float64(a) minus the plane mean summed in the workgroup's fixed order (restated on the host: action_opt_cases.block_sum_256)"""
    from pde_policylearning_amd import functional as F
    B = 2
    g = torch.Generator().manual_seed(23 + plane)
    v0 = 0.3 * torch.randn(B, plane, 1, generator=g, dtype=torch.float64)
    mean, std = _plane_stats(plane)
    md, sd = mean.to(dev), std.to(dev)
    for strided in (False, True):
        a = torch.full((B, plane), -7.0, device=dev)
        x = torch.full((B, 3, plane) if strided else (B, plane, 1, 1), -7.0, device=dev)
        F.ctrl_action_begin(v0.to(dev), md, sd, A.EPS, a, x, batch_stride=3 * plane if strided else None)
        assert K.bits_equal(a.cpu(), v0.reshape(B, plane).float())
        want_x = ((a.double() - md) / (sd + A.EPS)).float()
        assert K.bits_equal(x[:, 0] if strided else x.reshape(B, plane), want_x)
        if strided:
            assert bool((x[:, 1:] == -7.0).all())
    out = F.ctrl_action_finish(a, shape=(B, plane, 1))
    a64 = a.double().cpu().numpy()
    for b in range(B):
        want = a64[b] - A.block_sum_256(a64[b]) / float(plane)
        assert np.array_equal(out[b].cpu().numpy().ravel().view(np.int64), want.view(np.int64)), f"finish environment {b}"
        one = F.ctrl_action_finish(a[b:b + 1].contiguous(), shape=(1, plane, 1))
        assert K.bits_equal(one[0], out[b]), f"finish environment {b} depends on its batch position"


# ---------------------------------------------------------------------------------------------------------------------------
# 4: the lifting's input gradient
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [32, 64])
@pytest.mark.parametrize("cin", [1, 4])
def test_lifting_input_gradient(dev, cin, C):
    """fno_lifting_backward_dx against float64 under the rule (floor 1e-5) at planes of 128 and 1024 points, B in {1, 2};
    functional.lifting with a differentiable x returns the same dx and leaves dw, db as they are without it"""
    from pde_policylearning_amd import functional as F
    rows = []
    for plane in (128, 1024):
        for B in (1, 2):
            g = torch.Generator().manual_seed(100 * cin + C + plane + B)
            w, bias = torch.randn(C, cin, generator=g) / math.sqrt(cin), torch.randn(C, generator=g)
            x, dy = torch.randn(B, cin, plane // 32, 32, generator=g), torch.randn(B, C, plane // 32, 32, generator=g)
            want = torch.einsum("ci,bchw->bihw", w.double(), dy.double())
            ref32 = torch.einsum("ci,bchw->bihw", w, dy)
            dx = torch.empty(B, cin, plane // 32, 32, device=dev)
            wd, dyd = w.to(dev), dy.to(dev)
            F._call("lifting_backward_dx", dev, "fno_lifting_backward_dx", B, cin, C, plane, dyd, wd, dx, F.STREAM)
            rows.append((f"cin={cin} C={C} plane={plane} B={B} dx", A.rel_err(dx, want), A.rel_err(ref32, want), A.FLOOR))
            grads = []
            for need in (True, False):
                xl = x.to(dev).requires_grad_(need)
                wl, bl = wd.clone().requires_grad_(True), bias.to(dev).requires_grad_(True)
                y = F.lifting(xl, wl, bl)
                y.backward(dyd)
                grads.append((xl.grad, wl.grad, bl.grad))
            assert grads[1][0] is None and K.bits_equal(grads[0][0], dx), "functional.lifting's dx is not the entry point's"
            assert K.bits_equal(grads[0][1], grads[1][1]) and K.bits_equal(grads[0][2], grads[1][2]), "dw / db changed with dx"
            xs = x.to(dev).requires_grad_(True)
            F.lifting_per_sample_bias(xs, wd, bias.to(dev)[None].expand(B, C).contiguous()).backward(dyd)
            assert K.bits_equal(xs.grad, dx), "lifting_per_sample_bias's dx is not the entry point's"
    A.judge(f"lifting dx cin={cin} C={C}", rows)


# ---------------------------------------------------------------------------------------------------------------------------
# 5: the observer's input gradient
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def observer_fixture(dev):
    model = A.observer()
    p32, p64 = A.params_of(model), A.params_of(model, torch.float64)
    mean, std = A.stats()
    return model.to(dev).eval(), p32, p64, mean, std


def _input_gradient(p, x, mean, std, dtype):
    """dL/dx at reg = 0 from the oracle in `dtype` on the float32 input x (Nx, Nz): dy in closed form from its own output"""
    xl = x.to(dtype).clone().requires_grad_(True)
    y = A.forward(p, xl[None, :, :, None, None], A.RE)
    _, _, _, dy = A.objective_closed(y.detach()[0, :, :, :, 0], torch.zeros(A.NX, A.NZ), mean, std, 0.0)
    (dx,) = torch.autograd.grad(y, xl, dy.to(dtype)[None, :, :, :, None])
    return dx.double()


@pytest.mark.parametrize("B", [1, 2])
def test_observer_input_gradient(dev, observer_fixture, B):
    """the fixture observer, dy from the objective at reg = 0: dx against float64 autograd of the oracle under the rule with
    floor 1e-5; the launch log shows the lifting's forward kernel and k_lift_dx, i.e. the front stayed on the engine"""
    from pde_policylearning_amd import _lib, functional as F
    model, p32, p64, mean, std = observer_fixture
    for prm in model.parameters():
        prm.requires_grad_(False)
    md, sd = mean.reshape(-1).to(dev), std.reshape(-1).to(dev)
    a = torch.empty(B, A.NX * A.NZ, device=dev)
    x = torch.zeros(B, A.NX, A.NZ, 1, 1, device=dev).requires_grad_(True)
    F.ctrl_action_begin(A.start_action(B).to(dev), md, sd, A.EPS, a, x)
    re = torch.full((B,), A.RE, device=dev)
    with _lib.launch_log() as log:
        y = model(x, re)
        assert tuple(y.shape) == (B, A.PLANES, A.NX, A.NZ, 1)
        _, dy = F.ctrl_action_objective(y.detach(), a, md, sd, A.EPS, reg=0.0)
        (dx,) = torch.autograd.grad(y, x, dy.view(y.shape))
    names = [r["name"] for r in log.records]
    assert "k_pw_fwd_lift" in names and "k_lift_dx" in names, f"the observer's front left the engine: {sorted(set(names))}"
    rows = []
    for b in range(B):
        xb = x.detach()[b, :, :, 0, 0].cpu()
        want = _input_gradient(p64, xb, mean, std, torch.float64)
        rows.append((f"[{b}] dL/dx at reg = 0", A.rel_err(dx[b, :, :, 0, 0], want), A.rel_err(_input_gradient(p32, xb, mean, std, torch.float32), want), A.FLOOR))
    A.judge(f"observer input gradient B={B}", rows)


# ---------------------------------------------------------------------------------------------------------------------------
# 6: the whole policy on ControlLoop
# ---------------------------------------------------------------------------------------------------------------------------
PLANE = 3                 # detect_plane of the loop tests
_RESTATED = {}


def _setup():
    g = R.Grid(32, 10, 32)
    states = [R.analytic_state(g, 32 + b, noise=0.05) for b in range(2)]
    mean, std = A.stats()
    return g, states, A.Norm(mean.numpy(), std.numpy()), mean, std


def _restated(observer_fixture, start, reg):
    """(float64, reference-dtype) restatements from the GPU's own start action of one environment (float64 (Nx, Nz)), cached"""
    _, p32, p64, mean, std = observer_fixture
    key = (start.numpy().tobytes(), reg)
    if key not in _RESTATED:
        _RESTATED[key] = (A.policy_torch(p64, start, mean, std, -1.0, reg, A.EPOCHS, False),
                          A.policy_torch(p32, start, mean, std, -1.0, reg, A.EPOCHS, True))
    return _RESTATED[key]


def _gpu_record(pol, b):
    start = pol.start[b].float().double().cpu()
    fin = pol.a[b].double().cpu().reshape(start.shape)
    return {"start": start, "a": fin, "disp": fin - start, "loss": pol.losses[:, b, 0].cpu(), "opV2": pol.opV2[b].cpu()}


@pytest.mark.parametrize("reg", [0.0, 0.1])
@pytest.mark.parametrize("B", [1, 2])
def test_policy_on_control_loop(dev, observer_fixture, B, reg):
    """two control iterations: displacement, per-epoch loss and final opV2 against the float64 restatement fed the GPU's own
    start action, under the rule; opV1 is opposition control bit for bit; state and dPdx after the step against the
    restated rollout fed the GPU's own actions, under the float64 floor rule, in the same table.  (The environment has
    Re = -1, which the policy hands to the observer as the reference would.)"""
    from pde_policylearning_amd.control import ControlLoop, OptimalObserverPolicy
    g, states, norm, mean, std = _setup()
    env = K.make_env(dev, g, states[:B], PLANE)
    pol = OptimalObserverPolicy(observer_fixture[0], norm, reg_weight=reg)
    loop = ControlLoop(env, pol, 1, explode_at=None)
    steps, rows, obs, acts, after = 2, [], [], [], []
    for t in range(steps):
        V0 = env.V.clone()
        loop.run(keep_actions=True, keep_observations=True)
        assert K.bits_equal(pol.opV1, -V0[:, :, PLANE, :]), "opV1 is not opposition control"
        assert K.bits_equal(pol.start, -V0[:, :, -PLANE, :]) and K.bits_equal(loop.actions[0], pol.opV2)
        assert tuple(pol.losses.shape) == (A.EPOCHS, B, 3)
        obs.append(K.to_np(loop.observations[0]))
        acts.append((K.to_np(pol.opV1), K.to_np(pol.opV2)))
        after.append(([K.to_np(x) for x in (env.U, env.V, env.W)], K.to_np(env.dPdx_dev)))
        for b in range(B):
            got = _gpu_record(pol, b)
            r64, r32 = _restated(observer_fixture, got["start"], reg)
            rows += A.policy_rows(f"it {t} [{b}]", got, r32, r64)
            parts = pol.losses[:, b].cpu()
            assert torch.allclose(parts[:, 0], parts[:, 1] + reg * parts[:, 2], rtol=4 * EPS64, atol=0.0)
    A.judge(f"policy on ControlLoop B={B} reg={reg:g}", rows)
    srows = []
    for b in range(B):
        mine = [(v1[b], v2[b]) for v1, v2 in acts]
        base = K.restated_rollout(g, states[b], steps, actions=mine)
        pert = K.restated_rollout(g, states[b], steps, actions=mine, perturb=21 + b)
        gpu = [{"state": tuple(x[b] for x in after[t][0]), "dPdx": float(after[t][1][b]), "obs": obs[t][b]} for t in range(steps)]
        srows += K.loop_rows(g, f"[{b}]", gpu, base, pert)
    judge_floor(A.LOG, f"optimal-observer policy B={B} reg={reg:g}: state", srows)


# ---------------------------------------------------------------------------------------------------------------------------
# 7: graph
# ---------------------------------------------------------------------------------------------------------------------------
def test_graph_equals_eager(dev, observer_fixture, tmp_path):
    """three iterations, B = 2: state, log, actions, observations and policy.losses bit for bit; the whole iteration, the ten
    epochs included, is one graph; load_state replaces the state tensors, the graph is rebuilt and again equals eager"""
    from pde_policylearning_amd.control import ControlLoop, OptimalObserverPolicy
    g, states, norm, _, _ = _setup()
    loops = [ControlLoop(K.make_env(dev, g, states, PLANE), OptimalObserverPolicy(observer_fixture[0], norm), 3, graph=gr, explode_at=None)
             for gr in (False, True)]
    res = [l.run(keep_actions=True, keep_observations=True) for l in loops]
    e, gph = loops
    for n in ("U", "V", "W", "dPdx_dev"):
        assert K.bits_equal(getattr(e.env, n), getattr(gph.env, n)), n
    assert K.bits_equal(e.log, gph.log) and K.bits_equal(e.actions, gph.actions) and K.bits_equal(e.observations, gph.observations)
    assert K.bits_equal(e.policy.losses, gph.policy.losses) and K.bits_equal(e.policy.a, gph.policy.a)
    assert res[0].infos == res[1].infos
    path = str(tmp_path / "state.mat")
    e.env.dump_state(path)
    first, dp0 = gph._graph, e.env.dPdx_dev.clone()
    for l in loops:
        l.env.load_state(path)
        l.env.dPdx_dev.copy_(dp0)
        l.run()
    assert gph._graph is not first, "the graph was not rebuilt after load_state"
    for n in ("U", "V", "W", "dPdx_dev"):
        assert K.bits_equal(getattr(e.env, n), getattr(gph.env, n)), n + " after load_state"
    assert K.bits_equal(e.log, gph.log) and K.bits_equal(e.policy.losses, gph.policy.losses)


# ---------------------------------------------------------------------------------------------------------------------------
# 8: ensemble
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reg", [0.0, 0.1])
def test_ensemble_member_solves_its_own_problem(dev, observer_fixture, reg):
    """environment b of B = 2 against its own B = 1 run, under the rule (budget from the restatements of that environment).
    Not bitwise: the kernels of this change are batch-position invariant, but the observer's GEMM tiling may depend on B."""
    from pde_policylearning_amd.control import ControlLoop, OptimalObserverPolicy
    g, states, norm, _, _ = _setup()

    def run(sts):
        pol = OptimalObserverPolicy(observer_fixture[0], norm, reg_weight=reg)
        ControlLoop(K.make_env(dev, g, sts, PLANE), pol, 1, explode_at=None).run()
        return pol
    both = run(states)
    rows = []
    for b in range(2):
        alone, mine = _gpu_record(run(states[b:b + 1]), 0), _gpu_record(both, b)
        assert torch.equal(alone["start"], mine["start"])
        r64, r32 = _restated(observer_fixture, mine["start"], reg)
        z = lambda r: r["opV2"] - (r["start"] - r["start"].mean())      # noqa: E731
        for name, f in (("displacement", lambda r: r["disp"]), ("loss per epoch", lambda r: r["loss"]), ("opV2 - zero-mean start", z)):
            rows.append((f"[{b}] of 2 against B = 1: {name}", A.rel_err(f(mine), f(alone)), A.rel_err(f(r32), f(r64)), A.FLOOR))
    A.judge(f"ensemble reg={reg:g}", rows)
