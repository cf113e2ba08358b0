"""The optimal-policy-observer policy on the GPU (csrc/k_policy_opt.h, functional.ctrl_policy_*, PolicyModel2D,
FusedAdam.reset_state, control.PolicyObserverPolicy): the three kernels piece by piece, the objective through the new wrapper,
one epoch's parameter gradients, two control iterations teacher-forced epoch by epoch, the reference's zero initialisation,
graph against eager.  The rule, the fixture and the restatements live in tests/policy_opt_cases.py; every figure goes to
profiles/r17_policy_opt_errors.txt before it is asserted."""
import numpy as np
import pytest
import torch

from tests import action_opt_cases as A
from tests import chanflow_step_reference as R
from tests import control_loop_cases as K
from tests import policy_opt_cases as C
from tests.judging import dev  # noqa: F401

pytestmark = pytest.mark.gpu
PLANES = [1024, 1020, 257, 1]
DETECT = 3                 # detect_plane of the loop tests


def _rand(shape, seed, dtype=torch.float32, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return scale * torch.randn(*shape, generator=g, dtype=dtype)


# ---------------------------------------------------------------------------------------------------------------------------
# 1, 2: the kernels
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plane", PLANES)
@pytest.mark.parametrize("B", [1, 3])
def test_begin_and_compose(dev, B, plane):
    """a0 = float32(opV2_0), pin = float32(p2), x = a0 + res and opV2 = float64(x), bit for bit"""
    from pde_policylearning_amd import functional as F
    v0, p2 = _rand((B, plane, 1), 10 * B + plane, torch.float64, 0.3), _rand((B, plane, 1), 11 * B + plane, torch.float64, 2.0)
    res = _rand((B, plane, 1, 1, 1), 12 * B + plane, scale=0.05)
    a0, pin, x = (torch.full((B, plane), float("nan"), device=dev) for _ in range(3))
    opV2 = torch.full((B, plane, 1), float("nan"), dtype=torch.float64, device=dev)
    F.ctrl_policy_begin(v0.to(dev), p2.to(dev), a0, pin)
    F.ctrl_policy_compose(a0, res.to(dev), x, opV2)
    assert K.bits_equal(a0.cpu(), v0.float().reshape(B, plane)) and K.bits_equal(pin.cpu(), p2.float().reshape(B, plane))
    want = v0.float().reshape(B, plane) + res.reshape(B, plane)
    assert K.bits_equal(x.cpu(), want) and K.bits_equal(opV2.cpu(), want.double().reshape(B, plane, 1))


@pytest.mark.parametrize("plane", PLANES)
@pytest.mark.parametrize("B", [1, 3])
def test_grad(dev, B, plane):
    """g within one float32 ulp of the float64 closed form (the compiler may contract the multiply-add), for reg 0 and 0.1;
    g == dx bit for bit where na == 0 (the last environment's x is zero)"""
    from pde_policylearning_amd import functional as F
    dx, x = _rand((B, plane), 20 * B + plane, scale=1e-3), _rand((B, plane), 21 * B + plane, scale=0.3)
    x[-1] = 0.0
    dx[-1, 0] = -0.0
    parts = torch.zeros(B, 3, dtype=torch.float64)
    parts[:, 2] = x.double().norm(dim=1)
    lines, bad, worsts = [], [], []
    for reg in (0.0, 0.1):
        g = F.ctrl_policy_grad(dx.to(dev), x.to(dev), parts.to(dev), reg=reg).cpu()
        want = C.g_closed(dx, x, reg)
        ulp = torch.from_numpy(np.spacing(np.abs(want.float().numpy()))).double()
        worst = float(((g.double() - want).abs() / ulp).max())
        lines.append(f"B={B} plane={plane} reg={reg:g}: max |g - closed form| = {worst:.3f} ulp")
        print(lines[-1])
        worsts.append(worst)
        if not K.bits_equal(g[-1], dx[-1]):
            bad.append(f"reg={reg:g}: g != dx where na == 0")
        if reg == 0.0 and not K.bits_equal(g, dx):
            bad.append("reg=0: g != dx")
    C.log_block(f"grad B={B} plane={plane}", lines + bad)
    assert not bad and all(w <= 1.0 for w in worsts), lines + bad


# ---------------------------------------------------------------------------------------------------------------------------
# 3: the objective through the new wrapper
# ---------------------------------------------------------------------------------------------------------------------------
def test_objective_with_unit_statistics(dev):
    """nf, na and dy against float64 torch on one odd plane (257, P = 3, B = 3): parts under control_loop_cases.bound of a
    second summation order, dy within one float32 ulp of float32(y / nf): unit statistics change nothing"""
    import math
    from pde_policylearning_amd import functional as F
    B, P, plane = 3, 3, 257
    y, x = _rand((B, P, plane), 31), _rand((B, plane, 1, 1), 32, scale=0.3)
    parts, dy = F.ctrl_policy_objective(y.to(dev), x.to(dev), reg=0.1)
    parts, dy = parts.cpu(), dy.cpu()
    lines = []
    for b in range(B):
        yy, xx = y[b].double().numpy().ravel(), x[b].double().numpy().ravel()
        nf, na = math.sqrt(math.fsum(yy * yy)), math.sqrt(math.fsum(xx * xx))
        floor = max(abs(math.sqrt(float((yy * yy).sum())) - nf) / nf, abs(math.sqrt(float((xx * xx).sum())) - na) / na)
        for name, got, want in (("field_norm", parts[b, 1], nf), ("action_norm", parts[b, 2], na), ("loss", parts[b, 0], nf + 0.1 * na)):
            err = abs(float(got) - want) / want
            lines.append(f"[{b}] {name:12s} rel {err:.3e}   bound {K.bound(floor):.3e}   {'ok' if err <= K.bound(floor) else 'MISS'}")
        want = (y[b].double() / nf)
        ulp = torch.from_numpy(np.spacing(np.abs(want.float().numpy()))).double()
        worst = float(((dy[b].double() - want).abs() / ulp).max())
        lines.append(f"[{b}] dy max {worst:.3f} ulp   {'ok' if worst <= 1.0 else 'MISS'}")
    for l in lines:
        print(l)
    C.log_block("objective through ctrl_policy_objective B=3 P=3 plane=257", lines)
    assert not [l for l in lines if l.endswith("MISS")], lines


# ---------------------------------------------------------------------------------------------------------------------------
# the policy on an environment
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def nets():
    """the observer (shared: bind() freezes it, which every case wants) and its state dict; policies are built per case"""
    obs = A.observer()
    return obs, {k: v.clone() for k, v in obs.state_dict().items()}


def _states(B):
    g = R.Grid(32, 10, 32)
    return g, [R.analytic_state(g, 32 + b, noise=0.05) for b in range(B)]


def _policy_state(pol):
    """the policy's parameters as a CPU state dict (through state_dict(): the optimizer's hook keeps dead slices current)"""
    return {k: v.detach().cpu().clone() for k, v in pol.policy_model.state_dict().items()}


def _grads(pol):
    return {k: p.grad.detach().cpu().clone() for k, p in pol.policy_model.named_parameters()}


def _moments(pol):
    m, v = pol.optimizer.full_moments()
    return m.detach().cpu().clone(), v.detach().cpu().clone()


def _record(pol):
    p = pol.env.Nx, pol.env.Nz
    B = pol.env.B
    return {"res": pol.res.detach().reshape(B, *p).double().cpu(), "x": pol.x.detach().reshape(B, *p).double().cpu(),
            "g": pol.g.reshape(B, *p).double().cpu(), "dx": pol.dx.detach().reshape(B, *p).double().cpu(), "grads": _grads(pol)}


def _bound(dev, nets, states, g, width, reg, zero_init=False, graph=False, steps=1):
    from pde_policylearning_amd.control import ControlLoop, PolicyObserverPolicy
    pol = PolicyObserverPolicy(C.policy_model(width, zero_init=zero_init), nets[0], reg_weight=reg)
    loop = ControlLoop(K.make_env(dev, g, states, DETECT), pol, steps, graph=graph, explode_at=None)
    return loop, pol


def _dead_slices_zero(pol, grads):
    for m in pol.policy_model.pred_net.sp_convs:
        k = m.__dict__.get("_live_last")
        assert k is not None and k < m.modes3, "the fixture has no dead slice"
        for j in (1, 2, 3, 4):
            name = [n for n, p in pol.policy_model.named_parameters() if p is getattr(m, f"weights{j}")][0]
            assert not torch.view_as_real(grads[name][..., k:].resolve_conj()).any(), f"dead slice of d {name} is not zero"


# ---------------------------------------------------------------------------------------------------------------------------
# 4: one epoch's parameter gradients
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", C.WIDTHS)
@pytest.mark.parametrize("reg", [0.0, 0.1])
@pytest.mark.parametrize("B", [1, 2])
def test_one_epoch_gradients(dev, nets, B, reg, width):
    """begin() and epoch(0) at a non-zero initialisation: res, x, the three loss parts, dx, g and EVERY parameter gradient on
    its own under the rule against the float64 oracle; dead last-dimension slices of the spectral gradients exactly zero;
    B = 2 equals the sum of the two B = 1 gradients under the rule (budget: the float32 oracle's error at B = 2)"""
    g, states = _states(B)

    def run(sts):
        loop, pol = _bound(dev, nets, sts, g, width, reg)
        pp = _policy_state(pol)
        loop.observe()
        pol.begin(loop.p2)
        pol.epoch(0)
        return pol, pp
    pol, pp = run(states)
    a0, pin = pol.a0.reshape(B, 32, 32).cpu(), pol.pin.reshape(B, 32, 32).cpu()
    assert K.bits_equal(a0, (-pol.env.V[:, :, -DETECT, :]).float().cpu())
    got = _record(pol)
    got["parts"] = pol.losses[0].cpu()
    r64, r32 = (C.epoch_oracle(pp, nets[1], a0, pin, -1.0, reg, dt, width) for dt in (torch.float64, torch.float32))
    tag = f"B={B} reg={reg:g} width={width}"
    rows = C.epoch_rows(tag, got, r32, r64)
    want = C.dx_oracle(nets[1], pol.x.detach().reshape(B, 32, 32).cpu(), -1.0, torch.float64)
    rows.append((f"{tag} dx", C.rel_err(got["dx"], want),
                 C.rel_err(C.dx_oracle(nets[1], pol.x.detach().reshape(B, 32, 32).cpu(), -1.0, torch.float32), want), C.FLOOR))
    _dead_slices_zero(pol, got["grads"])
    if B == 2:
        singles = [run(states[b:b + 1])[0] for b in range(2)]
        for k in C.KEYS:
            view = lambda t: torch.view_as_real(t.resolve_conj()) if t.is_complex() else t      # noqa: E731
            both = view(got["grads"][k]).double()
            summed = sum(view(_grads(s)[k]).double() for s in singles)
            rows.append((f"{tag} d {k}: B = 2 against the sum of two B = 1", C.rel_err(both, summed),
                         C.rel_err(view(r32["grads"][k]), view(r64["grads"][k])), C.FLOOR))
    C.judge(f"one epoch {tag}", rows)


# ---------------------------------------------------------------------------------------------------------------------------
# 5: two control iterations, eager, teacher-forced
# ---------------------------------------------------------------------------------------------------------------------------
def test_two_iterations_teacher_forced(dev, nets):
    """B = 2, reg = 0.1, width 64, two control iterations on ControlLoop, the policy's begin / epoch(k) wrapped to download its
    state between them.  Every epoch against the oracles from the engine's own parameters at the start of that epoch; every
    Adam step against the restatement fed the engine's gradients and moments, the moments fresh at the first epoch of both
    iterations; opV1 opposition control and the applied opV2 the last epoch's x as float64, bit for bit; dead slices of the
    spectral weights bit-identical to their initial values after both iterations"""
    from pde_policylearning_amd.control import PolicyObserverPolicy
    B, reg, width = 2, 0.1, 64
    g, states = _states(B)
    trace = []

    class Recording(PolicyObserverPolicy):
        def begin(self, p2):
            super().begin(p2)
            trace.append({"V": self.env.V.clone(), "a0": self.a0.reshape(B, 32, 32).cpu(), "pin": self.pin.reshape(B, 32, 32).cpu(),
                          "count": self.optimizer.step_count, "moments": _moments(self), "epochs": []})

        def epoch(self, k):
            before = _policy_state(self), C_flat(self), _moments(self)
            super().epoch(k)
            rec = _record(self)
            rec.update(pp=before[0], p0=before[1], m0=before[2], grad_flat=self.bucket.flat.detach().cpu().clone(), p1=C_flat(self),
                       m1=_moments(self), parts=self.losses[k].cpu(), opV2=self.opV2.cpu().clone(), count=self.optimizer.step_count)
            trace[-1]["epochs"].append(rec)

    def C_flat(pol):
        return pol.optimizer.flat_param.detach().cpu().clone()
    from pde_policylearning_amd.control import ControlLoop
    pol = Recording(C.policy_model(width), nets[0], reg_weight=reg)
    loop = ControlLoop(K.make_env(dev, g, states, DETECT), pol, 1, explode_at=None)
    initial = _policy_state(pol)
    rows = []
    for it in range(2):
        loop.run(keep_actions=True)
        t = trace[it]
        assert K.bits_equal(pol.opV1, -t["V"][:, :, DETECT, :]), "opV1 is not opposition control"
        assert K.bits_equal(t["a0"], (-t["V"][:, :, -DETECT, :]).float().cpu())
        assert t["count"] == 0 and not t["moments"][0].any() and not t["moments"][1].any(), "the optimizer did not restart"
        last = t["epochs"][-1]
        assert K.bits_equal(loop.actions[0].cpu(), last["opV2"]) and K.bits_equal(last["opV2"], last["x"].reshape(last["opV2"].shape))
        assert K.bits_equal(last["x"].float(), t["a0"] + last["res"].float()), "the applied action is not the last forward's"
        for k, e in enumerate(t["epochs"]):
            assert e["count"] == k + 1
            r64, r32 = (C.epoch_oracle(e["pp"], nets[1], t["a0"], t["pin"], -1.0, reg, dt, width) for dt in (torch.float64, torch.float32))
            rows += C.epoch_rows(f"it {it} epoch {k}", e, r32, r64)
            rows += C.adam_rows(f"it {it} epoch {k}", e["p0"], (e["p1"],) + e["m1"], e["grad_flat"], *e["m0"], k + 1)
    C.judge("two control iterations, teacher-forced, B=2 reg=0.1", rows)
    final = _policy_state(pol)
    for m in pol.policy_model.pred_net.sp_convs:
        k = m.__dict__["_live_last"]
        for j in (1, 2, 3, 4):
            name = [n for n, p in pol.policy_model.named_parameters() if p is getattr(m, f"weights{j}")][0]
            assert K.bits_equal(torch.view_as_real(final[name][..., k:].resolve_conj()), torch.view_as_real(initial[name][..., k:].resolve_conj())), name
            assert not torch.equal(final[name][..., :k], initial[name][..., :k]), f"{name}: the live slice did not train"


# ---------------------------------------------------------------------------------------------------------------------------
# 6: the reference's zero initialisation
# ---------------------------------------------------------------------------------------------------------------------------
def test_zero_init_run(dev, nets):
    """two iterations from the reference's zero initialisation: every parameter but pred_net.fc2.bias is exactly 0.0, res is a
    uniform plane (so opV2 - a0 is uniform up to the one rounding of x = a0 + res)"""
    g, states = _states(1)
    loop, pol = _bound(dev, nets, states, g, 64, 0.1, zero_init=True)
    for it in range(2):
        loop.run()
        res = pol.res.detach().flatten()
        assert bool((res == res[0]).all()), "res is not uniform"
        x = pol.x.detach().flatten()
        assert K.bits_equal(x, pol.a0.flatten() + res) and K.bits_equal(pol.opV2.flatten(), x.double())
        off = pol.opV2.flatten() - pol.a0.flatten().double()
        half_ulp = torch.from_numpy(np.spacing(np.abs(x.cpu().numpy()))).double().to(dev) / 2
        assert bool(((off - res[0].double()).abs() <= half_ulp).all())
    for k, v in _policy_state(pol).items():
        zero = not (torch.view_as_real(v).any() if v.is_complex() else v.any())
        assert zero == (k != "pred_net.fc2.bias"), k
    assert float(res[0]) != 0.0 and float(pol.policy_model.pred_net.fc2.bias.detach()) != 0.0, "the head's bias did not train"


# ---------------------------------------------------------------------------------------------------------------------------
# 7: graph
# ---------------------------------------------------------------------------------------------------------------------------
def test_graph_equals_eager(dev, nets, monkeypatch):
    """three iterations, B = 2: state, log, actions, policy.losses, every policy parameter and the moments bit for bit; the
    parameters before the first replay equal the ones handed in, i.e. the capture's warm-up run did not train"""
    from pde_policylearning_amd import functional as F
    g, states = _states(2)
    handed = {k: v.clone() for k, v in C.policy_model(64).state_dict().items()}
    seen = []
    replay = F.GraphedControlLoop.replay

    def first_replay(self):
        if not seen:
            seen.append((_policy_state(gph.policy), _moments(gph.policy)))
        replay(self)
    monkeypatch.setattr(F.GraphedControlLoop, "replay", first_replay)
    loops = [_bound(dev, nets, states, g, 64, 0.1, graph=gr, steps=3)[0] for gr in (False, True)]
    e, gph = loops
    res = [l.run(keep_actions=True) for l in loops]
    assert seen and all(K.bits_equal(torch.view_as_real(v.resolve_conj()) if v.is_complex() else v,
                                     torch.view_as_real(handed[k]) if v.is_complex() else handed[k]) for k, v in seen[0][0].items())
    assert not seen[0][1][0].any() and not seen[0][1][1].any()
    for n in ("U", "V", "W", "dPdx_dev"):
        assert K.bits_equal(getattr(e.env, n), getattr(gph.env, n)), n
    assert K.bits_equal(e.log, gph.log) and K.bits_equal(e.actions, gph.actions)
    assert K.bits_equal(e.policy.losses, gph.policy.losses)
    assert K.bits_equal(e.policy.optimizer.flat_param, gph.policy.optimizer.flat_param)
    assert K.bits_equal(e.policy.optimizer.exp_avg, gph.policy.optimizer.exp_avg)
    assert K.bits_equal(e.policy.optimizer.exp_avg_sq, gph.policy.optimizer.exp_avg_sq)
    assert res[0].infos == res[1].infos
    assert not torch.equal(_policy_state(e.policy)["pred_net.fc1.weight"], handed["pred_net.fc1.weight"]), "the policy did not train"
