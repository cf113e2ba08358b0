"""Host side of the optimal-policy-observer policy (no GPU): PolicyModel2D's surface, the closed forms the kernels evaluate
against torch autograd of the reference's expressions, the degeneracy of the reference's zero initialisation, the float32
restatement of the kernels' arithmetic and three planted faults under the comparison rule (tests/policy_opt_cases.py),
make_policy / the run plan, and the refusals of the new entry points, which happen before any HIP call."""
import functools
import inspect
import pickle

import numpy as np
import pytest
import torch

from tests import action_opt_cases as A
from tests import policy_opt_cases as C
from tests.test_control_loop_host import BASE_CONTROL, _plan

REGS = (0.0, 0.1)


@pytest.fixture(scope="module")
def lib():
    from pde_policylearning_amd import _lib
    return _lib.lib()


@functools.lru_cache(maxsize=None)
def _fixture(width=64, B=1):
    """observer and policy state dicts (float32), a start action and a raw wall pressure"""
    return A.observer().state_dict(), C.policy_model(width).state_dict(), C.planes(B, 5, 0.3), C.planes(B, 7, 2.0)


# ---------------------------------------------------------------------------------------------------------------------------
# 1: surface
# ---------------------------------------------------------------------------------------------------------------------------
def test_policy_model_surface():
    from pde_policylearning_amd.libs.models import pino_models
    from pde_policylearning_amd.libs.models.pino_models import PolicyModel2D
    sig = inspect.signature(PolicyModel2D.__init__)
    want = [("modes1", inspect.Parameter.empty), ("modes2", inspect.Parameter.empty), ("modes3", inspect.Parameter.empty), ("width", 16),
            ("fc_dim", 128), ("layers", None), ("in_dim", 4), ("out_dim", 1), ("act", "gelu"), ("pad_ratio", [0., 0.]),
            ("use_fourier_layer", False), ("zero_init", True)]
    assert [(n, p.default) for n, p in list(sig.parameters.items())[1:]] == want
    assert pino_models.PolicyModel2D is PolicyModel2D
    kw = dict(modes1=[4] * 4, modes2=[4] * 4, modes3=[4] * 4, fc_dim=128, layers=[64] * 5, in_dim=1, out_dim=1, pad_ratio=[0.0, 0.0625])
    with pytest.raises(NotImplementedError):
        PolicyModel2D(use_fourier_layer=True, **kw)
    with pytest.raises(ValueError, match="zero_init"):
        PolicyModel2D(zero_init="tail", **kw)
    torch.manual_seed(0)
    ref = PolicyModel2D(**kw)
    assert list(ref.state_dict().keys()) == C.KEYS
    assert tuple(ref.pred_net.fc2.weight.shape) == (1, 128)
    assert all(not torch.view_as_real(p).any() if p.is_complex() else not p.any() for p in ref.parameters()), "default: every parameter zero"
    head, free = PolicyModel2D(zero_init="head", **kw), PolicyModel2D(zero_init=False, **kw)
    for name, prm in head.named_parameters():
        assert bool(prm.abs().sum() == 0) == name.startswith("pred_net.fc2."), name
    assert all(bool(prm.abs().sum() > 0) for prm in free.parameters())
    back = pickle.loads(pickle.dumps(free))
    assert all(torch.equal(a, b) for a, b in zip(back.state_dict().values(), free.state_dict().values()))
    assert list(back.state_dict().keys()) == C.KEYS and back.in_dim == 1 and back.max_re == 1000


# ---------------------------------------------------------------------------------------------------------------------------
# 2: closed forms
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reg", REGS)
def test_closed_forms_equal_autograd_of_the_reference_expressions(reg):
    """dy = y / nf and g = dx + reg x / na in float64 against torch autograd of run_control.py:169-173 in float64, B = 2 (each
    environment its own norms)"""
    po, pp, a0, pin = _fixture(64, 2)
    r = C.epoch_oracle(pp, po, a0, pin, C.RE, reg, torch.float64, 64)
    o = C.oracle_params(po, torch.float64)
    x = r["x"][..., None, None].clone().requires_grad_(True)
    y = A.forward(o, x, C.RE)
    dy = torch.stack([C.dy_closed(y.detach()[b])[1] for b in range(2)])
    for b in range(2):
        assert abs(float(C.dy_closed(y.detach()[b])[0]) - float(r["parts"][b, 1])) <= 1e-12 * float(r["parts"][b, 1])
    (dx,) = torch.autograd.grad(y, x, dy)
    assert C.rel_err(dx[..., 0, 0], C.dx_oracle(po, r["x"], C.RE, torch.float64)) < 1e-12
    assert C.rel_err(C.g_closed(dx[..., 0, 0], r["x"], reg), r["g"]) < 1e-12
    assert torch.equal(r["parts"][:, 0], r["parts"][:, 1] + reg * r["parts"][:, 2])
    # an all-zero output and an all-zero action have zero subgradients, as torch.norm's
    assert not C.dy_closed(torch.zeros(3, 4, 4))[1].any()
    z = torch.zeros(1, 4, 4)
    assert torch.equal(C.g_closed(torch.ones(1, 4, 4), z, reg), torch.ones(1, 4, 4, dtype=torch.float64))


# ---------------------------------------------------------------------------------------------------------------------------
# 3: the reference's zero initialisation is degenerate
# ---------------------------------------------------------------------------------------------------------------------------
def test_zero_init_changes_the_head_bias_and_nothing_else():
    """the float64 restatement from zero init, two control iterations of three epochs with a new torch.optim.Adam each: only
    pred_net.fc2.bias ever changes, exactly, and res is a uniform plane"""
    po = A.observer().state_dict()
    pp = C.policy_model(64, zero_init=True).state_dict()
    p = {k: v.requires_grad_(True) for k, v in C.oracle_params(pp, torch.float64).items()}
    o = C.oracle_params(po, torch.float64)
    for it in range(2):
        a0, pin = C.planes(1, 20 + it, 0.3).double()[..., None, None], C.planes(1, 30 + it, 2.0).double()[..., None, None]
        opt = torch.optim.Adam(list(p.values()), lr=C.LR)
        for _ in range(C.EPOCHS):
            opt.zero_grad()
            res = C.policy_forward(p, pin, C.RE, 64)
            assert bool((res == res.flatten()[0]).all()), "res is not a uniform plane"
            x = a0 + res
            (torch.norm(A.forward(o, x, C.RE)) + 0.1 * torch.norm(x)).backward()
            opt.step()
    for k, v in p.items():
        zero = not (torch.view_as_real(v.detach()).any() if v.is_complex() else v.detach().any())
        assert zero == (k != "observer_head.fc2.bias"), k


# ---------------------------------------------------------------------------------------------------------------------------
# 4: the rule and three planted faults
# ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _epoch_runs(reg):
    po, pp, a0, pin = _fixture(64, 1)
    return (C.epoch_oracle(pp, po, a0, pin, C.RE, reg, torch.float64, 64), C.epoch_oracle(pp, po, a0, pin, C.RE, reg, torch.float32, 64))


def test_float32_restatement_passes_and_planted_faults_are_rejected():
    po, pp, a0, pin = _fixture(64, 1)
    reg = 0.1
    r64, r32 = _epoch_runs(reg)
    mine = C.epoch_kernels(pp, po, a0, pin, C.RE, reg, 64)
    C.judge("host: float32 restatement of the kernels' arithmetic", C.epoch_rows("epoch 0", mine, r32, r64), who="restated")
    # (a) the regulariser's term as x / na^2
    bad = C.epoch_kernels(pp, po, a0, pin, C.RE, reg, 64, na_squared=True)
    assert "fault g" in C.rejected(C.epoch_rows("fault", bad, r32, r64, grads=False))
    # (b) the applied action re-evaluated after the last step: parameters moved by one Adam step of the epoch's own gradient
    flat, g = C.flat_of(pp), C.flat_of(r64["grads"]).float()
    zeros = torch.zeros_like(flat)
    stepped, m1, v1 = C.adam_step(flat, g, zeros, zeros, 1, torch.float32)
    moved, off = {}, 0
    for k in C.KEYS:
        n = pp[k].numel() * (2 if pp[k].is_complex() else 1)
        seg = stepped[off:off + n]
        moved[k] = torch.view_as_complex(seg.view(*pp[k].shape, 2)) if pp[k].is_complex() else seg.view(pp[k].shape)
        off += n
    late = C.epoch_kernels(moved, po, a0, pin, C.RE, reg, 64)
    rows = C.epoch_rows("fault", late, r32, r64, keys=("res", "x"), grads=False)
    assert "fault res" in C.rejected(rows), rows
    # (c) Adam moments carried into the next control iteration: the first step of an iteration fed the previous moments
    g2 = g.roll(1)
    fresh = C.adam_step(stepped, g2, zeros, zeros, 1, torch.float32)
    assert not C.rejected(C.adam_rows("fresh", stepped, fresh, g2, zeros, zeros, 1))
    carried = C.adam_step(stepped, g2, m1, v1, 1, torch.float32)
    assert len(C.rejected(C.adam_rows("fault", stepped, carried, g2, zeros, zeros, 1))) == 3


# ---------------------------------------------------------------------------------------------------------------------------
# 5: make_policy and the run plan
# ---------------------------------------------------------------------------------------------------------------------------
FULLFIELD_CONTROL = (BASE_CONTROL.replace("policy_name: gt", "policy_name: optimal-policy-observer")
                     .replace("model_name: FNO2dObserver", "model_name: PINObserverFullField"))
POLICY_CONTROL = FULLFIELD_CONTROL + "policy_model_name: PolicyModel2D\n"


def test_make_policy_builds_the_policy_from_operands():
    from pde_policylearning_amd.control import PolicyObserverPolicy, make_policy
    pm, obs = C.policy_model(64), A.observer()
    pol = make_policy("optimal-policy-observer", policy_model=pm, observer=obs, epochs=4, reg_weight=0.0, re=200.0)
    assert isinstance(pol, PolicyObserverPolicy) and pol.name == "optimal-policy-observer" and pol.collects is False
    assert (pol.epochs, pol.lr, pol.reg, pol.re) == (4, 1e-4, 0.0, 200.0) and pol.policy_model is pm and pol.observer is obs
    dflt = PolicyObserverPolicy(pm, obs)
    assert (dflt.epochs, dflt.lr, dflt.reg, dflt.re) == (3, 1e-4, 0.1, None)
    with pytest.raises(NotImplementedError, match="model_timestep"):
        make_policy("optimal-policy-observer", policy_model=pm, observer=obs, model_timestep=2)
    with pytest.raises(ValueError, match="epochs"):
        PolicyObserverPolicy(pm, obs, epochs=0)


def test_refusals_say_what_to_pass():
    from pde_policylearning_amd.control import make_policy
    with pytest.raises(NotImplementedError, match="policy_model="):
        make_policy("optimal-policy-observer")
    with pytest.raises(NotImplementedError, match="policy_model="):
        make_policy("optimal-policy-observer", observer=A.observer())
    with pytest.raises(NotImplementedError, match="policy_model_name"):
        _plan(BASE_CONTROL.replace("policy_name: gt", "policy_name: optimal-policy-observer"))         # model_name: FNO2dObserver
    with pytest.raises(NotImplementedError, match="policy_model_name"):
        _plan(FULLFIELD_CONTROL)                                                                       # no policy_model_name key
    with pytest.raises(NotImplementedError, match="policy_model_name"):
        _plan(FULLFIELD_CONTROL + "policy_model_name: DDPG\n")
    with pytest.raises(NotImplementedError, match="policy_model_name"):
        _plan(POLICY_CONTROL + "env_name: NSControlEnv2D\n")
    with pytest.raises(NotImplementedError, match="model_timestep"):
        _plan(POLICY_CONTROL.replace("model_timestep: 1", "model_timestep: 2"))
    with pytest.raises(ValueError, match="load_model_name"):
        _plan(POLICY_CONTROL.replace("load_model_name: planes_channel180_minchan_28-RNO-reproduce.pth", "load_model_name:"))
    with pytest.raises(ValueError, match="policy_zero_init"):
        _plan(POLICY_CONTROL + "policy_zero_init: tail\n")


def test_run_plan_accepts_the_policy_and_builds_it(tmp_path):
    from pde_policylearning_amd import run_control as RC
    from pde_policylearning_amd.control import PolicyObserverPolicy
    from pde_policylearning_amd.libs.models.pino_models import PolicyModel2D
    plan = _plan(POLICY_CONTROL.replace("DATA_FOLDER: ./data/planes_channel180_minchan", "DATA_FOLDER:"), ["--ensemble", "2", "--graph"])
    assert plan.policy_name == "optimal-policy-observer" and plan.policy_model_name == "PolicyModel2D" and plan.steps == 201
    assert plan.ensemble == 2 and plan.graph is True and plan.collect_data is False and plan.policy_zero_init is True
    assert _plan(FULLFIELD_CONTROL, ["--policy_model_name", "PolicyModel2D", "--policy_zero_init", "head"]).policy_zero_init == "head"
    out = tmp_path / "out"
    out.mkdir()
    torch.save(A.observer(), str(out / "observer.pth"))
    text = (POLICY_CONTROL.replace("load_model_name: planes_channel180_minchan_28-RNO-reproduce.pth", "load_model_name: observer.pth")
            .replace("output_dir: ./outputs", f"output_dir: {out}").replace("modes: 12", "modes: 4"))
    pol = RC.make_plan_policy(_plan(text), device="cpu")
    assert isinstance(pol, PolicyObserverPolicy) and pol.observer.plane_num == A.PLANES and (pol.epochs, pol.lr, pol.reg) == (3, 1e-4, 0.1)
    pm = pol.policy_model
    assert isinstance(pm, PolicyModel2D) and pm.layers == [64] * 5 and pm.modes1 == [4] * 4 and pm.in_dim == 1
    assert pm.pad_ratio == [0.0, 0.0625] and pm.pred_net.fc1.out_features == 128 and not any(p.abs().sum() for p in pm.parameters())
    assert any(p.abs().sum() for p in RC.make_plan_policy(_plan(text + "policy_zero_init: false\n"), device="cpu").policy_model.parameters())
    torch.save(C.policy_model(32), str(out / "policy.pth"))
    loaded = RC.make_plan_policy(_plan(text + "load_policy_name: policy.pth\n"), device="cpu").policy_model
    assert loaded.layers == [32] * 5 and any(p.abs().sum() for p in loaded.parameters())


# ---------------------------------------------------------------------------------------------------------------------------
# 6: refusals
# ---------------------------------------------------------------------------------------------------------------------------
def test_entry_points_refuse_on_the_host(lib):
    """every bad argument is a negative code and a message before any HIP call (this machine has no GPU to call)"""
    buf = np.zeros(64, dtype=np.float64)
    p, err = buf.ctypes.data, lib.fno_last_error
    assert lib.fno_ctrl_policy_begin(0, 16, p, p, p, p, None) < 0 and b"batch" in err()
    assert lib.fno_ctrl_policy_begin(1, 0, p, p, p, p, None) < 0 and b"plane" in err()
    for k in range(4):
        args = [p] * 4
        args[k] = None
        assert lib.fno_ctrl_policy_begin(1, 16, *args, None) < 0 and b"null" in err()
        assert lib.fno_ctrl_policy_compose(1, 16, *args, None) < 0 and b"null" in err()
    assert lib.fno_ctrl_policy_begin(1, 16, p + 4, p, p, p, None) < 0 and b"misaligned" in err()
    assert lib.fno_ctrl_policy_begin(1, 16, p, p, p + 2, p, None) < 0 and b"misaligned" in err()
    assert lib.fno_ctrl_policy_compose(0, 16, p, p, p, p, None) < 0 and b"batch" in err()
    assert lib.fno_ctrl_policy_compose(1, 0, p, p, p, p, None) < 0 and b"plane" in err()
    assert lib.fno_ctrl_policy_compose(1, 16, p, p, p, p + 4, None) < 0 and b"misaligned" in err()
    assert lib.fno_ctrl_policy_grad(0, 16, p, p, p, 0.1, p, None) < 0 and b"batch" in err()
    assert lib.fno_ctrl_policy_grad(1, 0, p, p, p, 0.1, p, None) < 0 and b"plane" in err()
    for k in range(4):
        args = [p, p, p, 0.1, p]
        args[k + (k == 3)] = None
        assert lib.fno_ctrl_policy_grad(1, 16, *args, None) < 0 and b"null" in err()
    assert lib.fno_ctrl_policy_grad(1, 16, p, p, p + 4, 0.1, p, None) < 0 and b"misaligned" in err()
    assert lib.fno_ctrl_policy_grad(1, 16, p, p, p, float("inf"), p, None) < 0 and b"reg" in err()


def test_wrappers_refuse_before_anything_is_launched():
    from pde_policylearning_amd import functional as F
    a, d = torch.zeros(2, 1024), torch.zeros(2, 32, 32, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="live on the GPU"):
        F.ctrl_policy_begin(d, d, a, a)
    with pytest.raises(RuntimeError, match="live on the GPU"):
        F.ctrl_policy_compose(a, a, a, d)
    with pytest.raises(RuntimeError, match="live on the GPU"):
        F.ctrl_policy_objective(torch.zeros(2, 3, 32, 32, 1), a)
    with pytest.raises(RuntimeError, match="live on the GPU"):
        F.ctrl_policy_grad(a, a, torch.zeros(2, 3, dtype=torch.float64))


def test_reset_state_needs_zero_weight_decay():
    """reset_state is exact only without weight decay; without one it restarts the count and the moments in place"""
    from pde_policylearning_amd.trainer import FlatGradBucket, FusedAdam
    lin = torch.nn.Linear(3, 2)
    with pytest.raises(RuntimeError, match="weight decay"):
        FusedAdam(FlatGradBucket(lin.parameters()), lr=1e-4, weight_decay=0.1).reset_state()
    opt = FusedAdam(FlatGradBucket(torch.nn.Linear(3, 2).parameters()), lr=1e-4)
    m, v = opt.exp_avg, opt.exp_avg_sq
    m.fill_(1.0), v.fill_(2.0)
    opt.step_count, opt._hp_log, opt._dead_step = 5, [(1, 1e-4, 0.9, 0.999, 1e-8, 0.0)], 2
    opt.reset_state()
    assert opt.exp_avg is m and opt.exp_avg_sq is v and not m.any() and not v.any()
    assert (opt.step_count, opt._hp_log, opt._dead_step) == (0, [], 0)
