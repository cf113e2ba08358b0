"""Host side of the optimal-observer policy (no GPU): the closed forms the kernels evaluate against torch autograd of the
reference's expressions, the condition that makes the fixture a valid Adam test, the float32 restatement and three planted
faults under the comparison rule (tests/action_opt_cases.py), make_policy / the run plan, and the refusals of the new entry
points, which happen before any HIP call."""
import functools

import numpy as np
import pytest
import torch

from tests import action_opt_cases as A
from tests.test_control_loop_host import BASE_CONTROL, _plan

REGS = (0.0, 0.1)


@pytest.fixture(scope="module")
def lib():
    from pde_policylearning_amd import _lib
    return _lib.lib()


@functools.lru_cache(maxsize=None)
def _fixture():
    m = A.observer()
    mean, std = A.stats()
    return A.params_of(m), A.params_of(m, torch.float64), mean, std, A.start_action(1)[0]


@functools.lru_cache(maxsize=None)
def _runs(reg):
    """the float64 and the reference-dtype restatements of the fixture at this reg_weight (computed once)"""
    p32, p64, mean, std, a0 = _fixture()
    return (A.policy_torch(p64, a0, mean, std, A.RE, reg, A.EPOCHS, False), A.policy_torch(p32, a0, mean, std, A.RE, reg, A.EPOCHS, True))


@pytest.mark.parametrize("reg", REGS)
def test_closed_forms_equal_autograd_of_the_reference_expressions(reg):
    """dy = field / nf * S and g = dx / S + reg a / na in float64, against torch autograd of run_control.py:211-220 in float64"""
    _, p64, mean, std, a0 = _fixture()
    a = a0.float().double().requires_grad_(True)
    L, y = A.reference_loss(p64, a, mean, std, A.RE, reg, False)
    y.retain_grad()
    L.backward()
    loss, nf, na, dy = A.objective_closed(y.detach()[0, :, :, :, 0], a.detach(), mean, std, reg)
    assert abs(float(loss) - float(L.detach())) <= 1e-12 * abs(float(L.detach()))
    assert A.rel_err(dy, y.grad[0, :, :, :, 0]) < 1e-12
    x = ((a.detach() - mean) / (std + A.EPS)).requires_grad_(True)
    yx = A.forward(p64, x[None, :, :, None, None], A.RE)
    (dx,) = torch.autograd.grad(yx, x, dy[None, :, :, :, None])
    assert A.rel_err(A.g_closed(dx, a.detach(), std, reg, na), a.grad) < 1e-12
    # an all-zero field and an all-zero action have zero subgradients, as torch.norm's
    zero = A.objective_closed(torch.zeros(A.PLANES, A.NX, A.NZ), torch.zeros(A.NX, A.NZ), torch.zeros_like(mean), std, reg)
    assert float(zero[0]) == 0.0 and not zero[3].any()
    assert not A.g_closed(torch.zeros(A.NX, A.NZ), torch.zeros(A.NX, A.NZ), std, reg, zero[2]).any()


@pytest.mark.parametrize("reg", REGS)
def test_fixture_keeps_every_gradient_entry_clear_of_the_float32_error(reg):
    """Adam's first step is lr * sign(g): min |g| / max |g| >= 20 x max |g32 - g64| / max |g64| at epoch 0 and at the last"""
    r64, r32 = _runs(reg)
    lines = []
    for k in (0, A.EPOCHS - 1):
        spread, err = A.sign_margin(r32["g"][k], r64["g"][k])
        lines.append(f"reg {reg:g} epoch {k}: min|g|/max|g| {spread:.3e}   max|g32 - g64|/max|g64| {err:.3e}   needs >= {20 * err:.3e}")
        print(lines[-1])
    A.log_block(f"fixture condition reg={reg:g} (CPU)", lines)
    for k in (0, A.EPOCHS - 1):
        spread, err = A.sign_margin(r32["g"][k], r64["g"][k])
        assert spread >= 20 * err, lines
    disp, act = float(r64["disp"].norm()), float(r64["a"].norm())
    assert 0.01 < disp / act < 0.1, "the final action is the start action to a few per cent: compare displacements"


@pytest.mark.parametrize("reg", REGS)
def test_float32_restatement_passes_and_planted_faults_are_rejected(reg):
    p32, _, mean, std, a0 = _fixture()
    r64, r32 = _runs(reg)
    run = lambda **kw: A.policy_restated(p32, a0, mean, std, A.RE, reg, A.EPOCHS, **kw)      # noqa: E731
    A.judge(f"restatement reg={reg:g} (CPU)", A.policy_rows("float32 restatement", run(), r32, r64), who="restated")
    # `S` dropped and the late bias corrections are tried at both reg values; a / na^2 only at 0.1: at reg = 0 the term it
    # corrupts is multiplied by zero, so there is nothing to reject (asserted: that run equals the unfaulted one)
    faults = [("bias correction off by one step", dict(bias_step_shift=-1)), ("S dropped from dy", dict(drop_S=True))]
    if reg == 0.0:
        assert torch.equal(run(na_squared=True)["a"], run()["a"])
    else:
        faults.append(("reg term a / na^2", dict(na_squared=True)))
    for name, kw in faults:
        rows = A.policy_rows(name, run(**kw), r32, r64)
        assert A.rejected(rows), f"the rule accepts the planted fault `{name}` at reg = {reg}: {rows}"


def test_block_sum_restatement_is_a_sum():
    v = np.random.default_rng(0).standard_normal(1020)
    assert abs(A.block_sum_256(v) - np.sum(v)) < 1e-12 and A.block_sum_256(np.ones(1)) == 1.0


# ---------------------------------------------------------------------------------------------------------------------------
# make_policy and the run plan
# ---------------------------------------------------------------------------------------------------------------------------
FULLFIELD_CONTROL = (BASE_CONTROL.replace("policy_name: gt", "policy_name: optimal-observer")
                     .replace("model_name: FNO2dObserver", "model_name: PINObserverFullField"))


def test_make_policy_builds_the_policy_from_operands():
    from pde_policylearning_amd.control import OptimalObserverPolicy, make_policy
    mean, std = A.stats()
    norm = A.Norm(mean.numpy(), std.numpy())
    pol = make_policy("optimal-observer", observer=A.observer(), v_norm=norm, epochs=4, reg_weight=0.0)
    assert isinstance(pol, OptimalObserverPolicy) and pol.name == "optimal-observer" and pol.collects is False
    assert (pol.epochs, pol.lr, pol.reg, pol.field_norm) == (4, 1e-3, 0.0, norm)
    dflt = OptimalObserverPolicy(A.observer(), norm)
    assert (dflt.epochs, dflt.lr, dflt.reg, dflt.re) == (10, 1e-3, 0.1, None)
    with pytest.raises(NotImplementedError, match="model_timestep"):
        make_policy("optimal-observer", observer=A.observer(), v_norm=norm, model_timestep=2)


def test_pinned_refusals_still_raise_and_say_what_to_pass():
    from pde_policylearning_amd.control import make_policy
    with pytest.raises(NotImplementedError, match="observer=.*v_norm="):
        make_policy("optimal-observer")
    with pytest.raises(NotImplementedError, match="PINObserverFullField"):
        _plan(BASE_CONTROL.replace("policy_name: gt", "policy_name: optimal-observer"))
    with pytest.raises(NotImplementedError):
        _plan(FULLFIELD_CONTROL + "env_name: NSControlEnv2D\n")
    for name in ("rand", "optimal-policy-observer"):
        with pytest.raises(NotImplementedError):
            make_policy(name)
        with pytest.raises(NotImplementedError):
            _plan(FULLFIELD_CONTROL.replace("optimal-observer", name))


def test_run_plan_accepts_a_fullfield_observer_yaml():
    plan = _plan(FULLFIELD_CONTROL, ["--ensemble", "3", "--graph"])
    assert plan.policy_name == "optimal-observer" and plan.model_name == "PINObserverFullField" and plan.steps == 201
    assert plan.ensemble == 3 and plan.graph is True and plan.collect_data is False and plan.collect_folder is None
    with pytest.raises(ValueError, match="load_model_name"):
        _plan(FULLFIELD_CONTROL.replace("load_model_name: planes_channel180_minchan_28-RNO-reproduce.pth", "load_model_name:"))
    with pytest.raises(ValueError, match="DATA_FOLDER"):
        _plan(FULLFIELD_CONTROL.replace("DATA_FOLDER: ./data/planes_channel180_minchan", "DATA_FOLDER:"))
    with pytest.raises(NotImplementedError, match="model_timestep"):
        _plan(FULLFIELD_CONTROL.replace("model_timestep: 1", "model_timestep: 2"))


def test_run_control_builds_the_policy_from_a_saved_observer_and_a_fullfield_dataset(tmp_path):
    """make_plan_policy on a tiny synthetic full-field dataset: the pickled observer is loaded, FullFieldNSDataset opens the
    folder, the action is encoded with bound_v_norm (the statistics of the wall plane V[:, -1, :]) and the planes decoded with
    v_field_norm, which is the same object"""
    from pde_policylearning_amd import run_control as RC
    from pde_policylearning_amd.control import OptimalObserverPolicy, write_metadata
    Nx, Ny, Nz = 32, 5, 32
    rng = np.random.default_rng(4)
    folder, out = tmp_path / "data", tmp_path / "out"
    folder.mkdir()
    out.mkdir()
    vm, vs = 0.05 * rng.standard_normal((Nx, Ny, Nz)), 0.2 + 0.1 * rng.random((Nx, Ny, Nz))
    pm, ps = rng.standard_normal((Nx, Nz)), 1.0 + rng.random((Nx, Nz))
    write_metadata(str(folder), 180.0, {"V_field": (vm, vs), "P_planes": (pm, ps)}, [3e-3])
    torch.save(A.observer(), str(out / "observer.pth"))
    plan = _plan(FULLFIELD_CONTROL.replace("load_model_name: planes_channel180_minchan_28-RNO-reproduce.pth", "load_model_name: observer.pth")
                 .replace("DATA_FOLDER: ./data/planes_channel180_minchan", f"DATA_FOLDER: {folder}")
                 .replace("output_dir: ./outputs", f"output_dir: {out}"))
    pol = RC.make_plan_policy(plan, device="cpu")
    assert isinstance(pol, OptimalObserverPolicy) and pol.observer.plane_num == A.PLANES and pol.observer.in_dim == 1
    assert pol.field_norm is pol.v_norm and (pol.epochs, pol.reg, pol.re) == (10, 0.1, None)
    assert np.array_equal(np.asarray(pol.v_norm.mean), vm[:, -1, :]) and np.array_equal(np.asarray(pol.v_norm.std), vs[:, -1, :])


# ---------------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------------
def test_entry_points_refuse_on_the_host(lib):
    """every bad argument is a negative code and a message before any HIP call (this machine has no GPU to call)"""
    buf = np.zeros(64, dtype=np.float64)
    p, err = buf.ctypes.data, lib.fno_last_error
    hyper = (1e-5, 0.1, 1e-3, 0.9, 0.999, 1e-8)
    assert lib.fno_ctrl_action_workspace_bytes(2, 3, 1024) == 2 * 3 * 2 * 8
    assert lib.fno_ctrl_action_workspace_bytes(1, 3, 1020) == 3 * 2 * 8 and lib.fno_ctrl_action_workspace_bytes(1, 1, 1) == 16
    assert lib.fno_ctrl_action_workspace_bytes(0, 3, 1024) == 0 and b"batch" in err()
    assert lib.fno_ctrl_action_workspace_bytes(1, 0, 1024) == 0 and b"planes" in err()
    assert lib.fno_ctrl_action_begin(0, 16, p, p, p, 1e-5, p, p, 16, None) < 0 and b"batch" in err()
    assert lib.fno_ctrl_action_begin(1, 16, p, p, p, 1e-5, p, p, 8, None) < 0 and b"stride" in err()
    assert lib.fno_ctrl_action_begin(1, 16, p, None, p, 1e-5, p, p, 16, None) < 0 and b"statistics" in err()
    assert lib.fno_ctrl_action_begin(1, 16, None, p, p, 1e-5, p, p, 16, None) < 0 and b"null" in err()
    assert lib.fno_ctrl_action_begin(1, 16, p + 4, p, p, 1e-5, p, p, 16, None) < 0 and b"misaligned" in err()
    assert lib.fno_ctrl_action_objective(1, 3, 16, p, p, p, p, 1e-5, 0.1, p, p, p, 8, None) < 0 and b"workspace" in err()
    assert lib.fno_ctrl_action_objective(1, 65, 16, p, p, p, p, 1e-5, 0.1, p, p, p, 16, None) < 0 and b"planes" in err()
    assert lib.fno_ctrl_action_objective(1, 3, 16, p, p, p, p, 1e-5, 0.1, None, p, p, 16, None) < 0 and b"null" in err()
    assert lib.fno_ctrl_action_objective(1, 3, 16, p, p, p, p, 1e-5, float("nan"), p, p, p, 16, None) < 0 and b"reg" in err()
    assert lib.fno_ctrl_action_objective(1, 3, 16, p, p, p, p, 1e-5, 0.1, p + 4, p, p, 16, None) < 0 and b"misaligned" in err()
    assert lib.fno_ctrl_action_update(1, 16, p, p, p, p, *hyper, 0, p, p, p, p, 16, None) < 0 and b"step" in err()
    assert lib.fno_ctrl_action_update(1, 16, p, p, p, p, *hyper, 1, p, None, p, p, 16, None) < 0 and b"null" in err()
    assert lib.fno_ctrl_action_update(1, 16, p, p, p, p, *hyper, 1, p, p, p, p, 15, None) < 0 and b"stride" in err()
    assert lib.fno_ctrl_action_update(1, 16, p, p, p, p, 1e-5, 0.1, 1e-3, 1.0, 0.999, 1e-8, 1, p, p, p, p, 16, None) < 0 and b"betas" in err()
    assert lib.fno_ctrl_action_finish(1, 0, p, p, None) < 0 and b"plane" in err()
    assert lib.fno_ctrl_action_finish(1, 16, p, None, None) < 0 and b"null" in err()
    assert lib.fno_ctrl_action_finish(1, 16, p, p + 4, None) < 0 and b"misaligned" in err()
    assert lib.fno_lifting_backward_dx(1, 5, 64, 1024, p, p, p, None) < 0 and b"input channels" in err()
    assert lib.fno_lifting_backward_dx(1, 1, 48, 1024, p, p, p, None) < 0 and b"32 or 64" in err()
    assert lib.fno_lifting_backward_dx(1, 1, 64, 1000, p, p, p, None) < 0 and b"128" in err()
    assert lib.fno_lifting_backward_dx(1, 1, 64, 1024, p, None, p, None) < 0 and b"null" in err()
    assert lib.fno_lifting_backward_dx(1, 1, 64, 1024, p + 4, p, p, None) < 0 and b"misaligned" in err()


def test_wrappers_refuse_before_anything_is_launched():
    from pde_policylearning_amd import functional as F
    mean, std = A.stats()
    a = torch.zeros(2, 1024)
    with pytest.raises(RuntimeError, match="live on the GPU"):
        F.ctrl_action_begin(torch.zeros(2, 32, 32, dtype=torch.float64), mean, std, 1e-5, a, torch.zeros(2, 32, 32, 1, 1))
    with pytest.raises(RuntimeError, match="live on the GPU"):
        F.ctrl_action_objective(torch.zeros(2, 3, 32, 32, 1), a, mean, std)
    with pytest.raises(RuntimeError, match="live on the GPU"):
        F.ctrl_action_update(torch.zeros(2, 1024), torch.zeros(2, 3, dtype=torch.float64), mean, std, 1e-5, a, a, a, a, 1)
    with pytest.raises(RuntimeError, match="live on the GPU"):
        F.ctrl_action_finish(a, shape=(2, 32, 32))
