"""Closed-loop control rollouts and dataset collection on the engine (reference: run_control.py).

One control iteration is
    action from the current observation -> [collect] -> rk3_step -> wall pressure of the new state -> diagnostics into the log
and nothing in it is copied to the host: the observation p2, the action, the state, dPdx and the (T, B, 13) log are device
tensors; the log is read every `check_every` iterations for the reference's "Control exploded!" test and once at the end for
`result.infos`.  The reference solves the pressure twice per iteration (get_boundary_pressures before the policy, again inside
step) on the same state with the same dPdx; here the observation of iteration i + 1 is the one iteration i ended with.

Policies map the observation p2 (B, Nx, Nz) float64 on the device to opV1, opV2 (B, Nx, Nz) float64 on the device:
GtPolicy (opposition control), UnmanipulatedPolicy, FnoPolicy / RnoPolicy (a trained observer between the two bridges
functional.ctrl_encode / ctrl_decode), OptimalObserverPolicy (Adam on the action itself through the full-field observer,
functional.ctrl_action_*), PolicyObserverPolicy (a policy network trained on line through the same observer,
functional.ctrl_policy_*).  Collector writes the reference's dataset format (run_control.py:234-293)."""
import os
import queue
import threading

import numpy as np
import torch

from . import functional as F

EXPLODE_DIV = 10.0          # run_control.py:294: abs(reward_div()) > 10
FIELDS = ("P_planes", "V_planes", "U_field", "V_field", "W_field", "du_dt")


# ---------------------------------------------------------------------------------------------------------------------------
# policies
# ---------------------------------------------------------------------------------------------------------------------------
class Policy:
    """bind(env) once, then act(p2) -> (opV1, opV2) per iteration, on persistent device tensors (so an iteration can be
    captured into a graph)"""
    name = "policy"
    collects = False            # run_control.py:45-46: only gt and unmanipulated runs may collect a dataset

    def bind(self, env):
        self.env = env
        shp = (env.B, env.Nx, env.Nz)
        self.opV1 = torch.zeros(shp, dtype=torch.float64, device=env.device)
        self.opV2 = torch.zeros(shp, dtype=torch.float64, device=env.device)
        return self

    def act(self, p2):
        raise NotImplementedError


class GtPolicy(Policy):
    """opposition control on both walls: minus the wall-normal velocity at `detect_plane` (gt_control)"""
    name, collects = "gt", True

    def __init__(self, detect_plane=None):
        self.detect_plane = detect_plane

    def act(self, p2):
        d = self.env.detect_plane if self.detect_plane is None else int(self.detect_plane)
        V = self.env.V
        torch.neg(V[:, :, d, :], out=self.opV1)
        torch.neg(V[:, :, -d, :], out=self.opV2)
        return self.opV1, self.opV2


class UnmanipulatedPolicy(Policy):
    """no control: zeros on both walls; the loop calls reset_init at iteration 0 (run_control.py:227-232)"""
    name, collects = "unmanipulated", True

    def act(self, p2):
        return self.opV1, self.opV2


def _stat(a, device):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64).reshape(-1)).to(device)


class _ObserverPolicy(Policy):
    """encode with the pressure statistics, run the observer under no_grad in eval(), decode with the velocity statistics
    (run_control.py:139-154; the attributes it names at :140,147 do not exist on its dataset, the intent is stated here).
    p_norm, v_norm: NormalizerGivenMeanStd (anything with mean, std, eps)."""

    def __init__(self, observer, p_norm, v_norm, zero_mean=False, scale=1.0, clip=0.0):
        self.observer, self.p_norm, self.v_norm = observer, p_norm, v_norm
        self.zero_mean, self.scale, self.clip = bool(zero_mean), float(scale), float(clip)

    def bind(self, env):
        super().bind(env)
        dev, plane = env.device, env.Nx * env.Nz
        # side effect on the caller's module: moved to the environment's device and left in eval().  OptimalObserverPolicy.bind
        # goes one step further and freezes the parameters (requires_grad_(False)); a caller that trains the observer
        # afterwards has to switch both back, and one that shares the module with other code should pass a copy.
        self.observer = self.observer.to(dev).eval()
        self.p_stats = (_stat(self.p_norm.mean, dev), _stat(self.p_norm.std, dev), float(self.p_norm.eps))
        self.v_stats = (_stat(self.v_norm.mean, dev), _stat(self.v_norm.std, dev), float(self.v_norm.eps))
        for n, s in (("pressure", self.p_stats), ("velocity", self.v_stats)):
            if s[0].numel() != plane or s[1].numel() != plane:
                raise RuntimeError(f"{type(self).__name__}: the {n} statistics have {s[0].numel()} / {s[1].numel()} points, the "
                                   f"observed plane {env.Nx} x {env.Nz} = {plane}")
        self.x = self._input(env)
        return self

    def act(self, p2):
        plane = self.env.Nx * self.env.Nz
        mean, std, eps = self.p_stats
        F.ctrl_encode(p2, mean, std, eps, out=self.x, batch_stride=self.x[0].numel())
        with torch.no_grad():
            y = self._model(self.x)
        if y.numel() != self.env.B * plane:
            raise RuntimeError(f"{type(self).__name__}: the observer returned {tuple(y.shape)} for {self.env.B} planes of {plane}")
        mean, std, eps = self.v_stats
        F.ctrl_decode(y.contiguous(), mean, std, eps, scale=self.scale, clip=self.clip, zero_mean=self.zero_mean,
                      out=(self.opV1, self.opV2))
        return self.opV1, self.opV2


class FnoPolicy(_ObserverPolicy):
    """FNO2dObserver as the controller.  The NCHW input (B, 3, Nx, Nz) is persistent: its two grid channels are filled once,
    ctrl_encode writes channel 0; no cat / permute / contiguous per iteration."""
    name = "fno"

    def _input(self, env):
        if getattr(self.observer, "use_v_plane", False):
            raise NotImplementedError("FnoPolicy: an observer with use_v_plane needs the previous action as an input")
        x = torch.empty((env.B, 3, env.Nx, env.Nz), dtype=torch.float32, device=env.device)
        x[:, 1:] = self.observer.get_grid((env.B, env.Nx, env.Nz), env.device).permute(0, 3, 1, 2)
        x[:, 0] = 0
        return x

    def _model(self, x):
        return self.observer.fno2d(x)


class RnoPolicy(_ObserverPolicy):
    """RNO2d as the controller on the (B, 1, Nx, Nz, 1) input (run_control.py:150-154)"""
    name = "rno"

    def _input(self, env):
        return torch.zeros((env.B, 1, env.Nx, env.Nz, 1), dtype=torch.float32, device=env.device)

    def _model(self, x):
        return self.observer(x, None)


class OptimalObserverPolicy(Policy):
    """The reference's `optimal-observer` (run_control.py:186-224): every control iteration starts from opposition control and
    takes `epochs` Adam steps on the upper-wall action itself, descending
        |decoded v-planes the full-field observer predicts from the action|_2 + reg_weight * |action|_2
    through the trained PINObserverFullField down to its input; opV1 is opposition control as it is, opV2 the optimised action
    minus its own plane mean.  Per environment b, S = std + eps:
        a = float32(opV2_0), fresh Adam state; per epoch  x = float32((float64(a) - mean) / S),  y = observer(x, Re) in float32,
        field = float64(y) * S + mean,  loss = |field| + reg |a| in float64,  g = float32(dL/dx / S + reg a / |a|),  Adam step.
    The objective (functional.ctrl_action_objective) hands the observer's backward its output gradient dy directly
    (torch.autograd.grad(y, x, dy)): no scalar torch loss is built, and everything around the observer is four engine kernels
    on persistent tensors, so the whole iteration is captured by ControlLoop(graph=True) on one stream.
    v_norm: the wall-plane normaliser the action is encoded with (FullFieldNSDataset.bound_v_norm); field_norm: the one the
    predicted planes are decoded with (the dataset's v_field_norm is the same object; default v_norm).  re: default env.Re.
    `losses`: the last iteration's (epochs, B, 3) device tensor, columns functional.ACTION_PARTS.
    Departures from the reference: (1) its forward before the loop (`initial_loss`, :195-206) computes a value nothing uses and
    is not run; the epoch-0 loss is what `losses[0]` holds.  (2) it calls torch.norm over the whole batch and its batch is 1;
    here every environment of an ensemble has its own norms, loss and Adam state, so environment b of B solves the problem
    its own B = 1 run solves.  (3) it leaves the observer's parameters collecting .grad that nothing reads; bind() puts the
    observer in eval() and freezes its parameters (requires_grad_(False)), so the backward skips the weight gradients it can.
    (4) g is assembled in float64 and rounded once; the reference accumulates two float32 contributions.
    The freeze of (3) is done in place on the module that was passed and is not undone: do not share one observer object
    between this policy and anything that expects its parameters to require grad (another policy, a trainer) - hand this
    policy its own copy (copy.deepcopy), or switch requires_grad back on afterwards.  model_timestep != 1 is refused by
    make_policy and by the run plan."""
    name, collects = "optimal-observer", False

    def __init__(self, observer, v_norm, epochs=10, lr=1e-3, reg_weight=0.1, re=None, field_norm=None):
        if int(epochs) < 1:
            raise ValueError(f"OptimalObserverPolicy: epochs must be at least 1 (got {epochs})")
        self.observer, self.v_norm, self.field_norm = observer, v_norm, v_norm if field_norm is None else field_norm
        self.epochs, self.lr, self.reg, self.re = int(epochs), float(lr), float(reg_weight), re

    def bind(self, env):
        super().bind(env)
        dev, B, plane = env.device, env.B, env.Nx * env.Nz
        obs = self.observer
        P = getattr(obs, "plane_num", None)
        if getattr(obs, "in_dim", None) != 1 or not isinstance(P, int) or P < 1:
            raise RuntimeError(f"OptimalObserverPolicy: the observer must take in_dim = 1 (the encoded wall plane) and return "
                               f"plane_num planes, as PINObserverFullField does (got in_dim = {getattr(obs, 'in_dim', None)}, "
                               f"plane_num = {P})")
        self.observer = obs.to(dev).eval()       # (see _ObserverPolicy.bind) and frozen: the loop differentiates to the input only
        for prm in self.observer.parameters():
            prm.requires_grad_(False)
        self.v_stats = (_stat(self.v_norm.mean, dev), _stat(self.v_norm.std, dev), float(self.v_norm.eps))
        self.f_stats = (_stat(self.field_norm.mean, dev), _stat(self.field_norm.std, dev), float(self.field_norm.eps))
        for n, s in (("wall-plane", self.v_stats), ("field", self.f_stats)):
            if s[0].numel() != plane or s[1].numel() != plane:
                raise RuntimeError(f"OptimalObserverPolicy: the {n} statistics have {s[0].numel()} / {s[1].numel()} points, the "
                                   f"controlled plane {env.Nx} x {env.Nz} = {plane}")
        f32 = lambda *shp: torch.zeros(shp, dtype=torch.float32, device=dev)      # noqa: E731
        self.P = P
        self.a, self.exp_avg, self.exp_avg_sq = f32(B, plane), f32(B, plane), f32(B, plane)
        self.x = f32(B, env.Nx, env.Nz, 1, 1).requires_grad_(True)                 # the persistent observer input: a leaf
        self.dy = f32(B, P, plane)
        self.start = torch.zeros((B, env.Nx, env.Nz), dtype=torch.float64, device=dev)
        self.losses = torch.zeros((self.epochs, B, len(F.ACTION_PARTS)), dtype=torch.float64, device=dev)
        self.ws = F.ctrl_action_workspace(B, P, plane, dev)
        self.re_t = torch.full((B,), float(env.Re if self.re is None else self.re), dtype=torch.float32, device=dev)
        return self

    def act(self, p2):
        env = self.env
        B, plane = env.B, env.Nx * env.Nz
        d = env.detect_plane
        torch.neg(env.V[:, :, d, :], out=self.opV1)
        torch.neg(env.V[:, :, -d, :], out=self.start)
        mean, std, eps = self.v_stats
        F.ctrl_action_begin(self.start, mean, std, eps, self.a, self.x)
        with torch.enable_grad():
            for k in range(self.epochs):
                y = self.observer(self.x, self.re_t)
                if y.numel() != B * self.P * plane:
                    raise RuntimeError(f"OptimalObserverPolicy: the observer returned {tuple(y.shape)} for {B} x {self.P} planes of {plane}")
                F.ctrl_action_objective(y.detach(), self.a, *self.f_stats, reg=self.reg, parts=self.losses[k], dy=self.dy, ws=self.ws)
                (dx,) = torch.autograd.grad(y, self.x, self.dy.view(y.shape))
                F.ctrl_action_update(dx, self.losses[k], mean, std, eps, self.a, self.exp_avg, self.exp_avg_sq, self.x, k + 1,
                                     reg=self.reg, lr=self.lr)
        F.ctrl_action_finish(self.a, out=self.opV2)
        return self.opV1, self.opV2


class PolicyObserverPolicy(Policy):
    """The reference's `optimal-policy-observer` (run_control.py:162-185): a neural policy (PolicyModel2D) maps the observed
    RAW wall pressure to a correction of the opposition-control action and is trained on line, inside every control
    iteration, by descending  |observer(action)|_2 + reg_weight * |action|_2  through the trained, frozen
    PINObserverFullField.  opV1 is opposition control as it is.  Per control iteration:
        begin():   opV1 = -V[detect], a0 = float32(-V[-detect]), pin = float32(p2) (functional.ctrl_policy_begin); the optimizer
                   restarts (FusedAdam.reset_state: the reference builds a NEW Adam per iteration, so fresh moments and step
                   count; the policy's parameters persist across iterations)
        epoch(k):  res = policy(pin, Re);  x = a0 + res, opV2 = float64(x) (ctrl_policy_compose; x a persistent leaf)
                   y = observer(x, Re): raw action in, raw planes out;  parts[k], dy = ctrl_policy_objective(y, x)
                   dx = autograd.grad(y, x, dy);  g = float32(dx + reg x / |x|) = dL/dres (ctrl_policy_grad)
                   zero the live gradients;  autograd.backward(res, g);  Adam step k + 1 (a host constant)
    act(p2) = begin() then epoch(0 .. epochs - 1).  The applied opV2 is the x of the LAST FORWARD, i.e. under the parameters
    after epochs - 1 steps (the reference's `opV2 = a0 + res` after its loop); the last step only shows in the next control
    iteration; no plane mean is removed.  `losses`: the last iteration's (epochs, B, 3) device tensor, columns
    functional.ACTION_PARTS.  re: default env.Re.
    Ensemble: ONE policy network serves all B environments; the objective is the sum over the environments of each
    environment's own nf_b + reg * na_b (the reference has B = 1 and one torch.norm), the parameter gradient the sum over b.
    Unlike OptimalObserverPolicy, a member of an ensemble is therefore NOT its own B = 1 run: the members train one network.
    Departures from the reference: (1) its forward pair before the loop computes a loss that is only printed and is not run
    (as OptimalObserverPolicy's (1)); (2) bind() puts the observer in eval() and freezes its parameters in place - the
    reference leaves them collecting .grad nothing reads; pass a copy if the module is shared (see OptimalObserverPolicy);
    (3) g is assembled in float64 and rounded once; (4) the policy's parameters are re-pointed at one flat buffer
    (FusedAdam), and the dead 11/12 of its spectral weights at T = 1 are neither stepped nor read in a control iteration.
    Graph: Adam restarts at step 1 every iteration, so the step numbers are capture-time constants and ControlLoop(graph=True)
    captures the whole iteration; state_tensors() names what the capture's eager warm-up must not leave changed."""
    name, collects = "optimal-policy-observer", False

    def __init__(self, policy_model, observer, epochs=3, lr=1e-4, reg_weight=0.1, re=None):
        if int(epochs) < 1:
            raise ValueError(f"PolicyObserverPolicy: epochs must be at least 1 (got {epochs})")
        self.policy_model, self.observer = policy_model, observer
        self.epochs, self.lr, self.reg, self.re = int(epochs), float(lr), float(reg_weight), re

    def bind(self, env):
        from .trainer import FlatGradBucket, FusedAdam
        super().bind(env)
        dev, B, plane = env.device, env.B, env.Nx * env.Nz
        obs, pm = self.observer, self.policy_model
        P = getattr(obs, "plane_num", None)
        if getattr(obs, "in_dim", None) != 1 or not isinstance(P, int) or P < 1:
            raise RuntimeError(f"PolicyObserverPolicy: the observer must take in_dim = 1 (the wall action) and return plane_num "
                               f"planes, as PINObserverFullField does (got in_dim = {getattr(obs, 'in_dim', None)}, plane_num = {P})")
        head = getattr(getattr(pm, "pred_net", None), "fc2", None)
        if getattr(pm, "in_dim", None) != 1 or getattr(head, "out_features", None) != 1:
            raise RuntimeError(f"PolicyObserverPolicy: the policy model must take in_dim = 1 (the wall pressure) and return one "
                               f"channel, as PolicyModel2D(in_dim=1, out_dim=1) does (got in_dim = {getattr(pm, 'in_dim', None)}, "
                               f"outputs = {getattr(head, 'out_features', None)})")
        self.observer = obs.to(dev).eval()       # (see _ObserverPolicy.bind) and frozen: the loop differentiates to the input only
        for prm in self.observer.parameters():
            prm.requires_grad_(False)
        self.policy_model = pm = pm.to(dev)
        f32 = lambda *shp: torch.zeros(shp, dtype=torch.float32, device=dev)      # noqa: E731
        self.P = P
        self.a0, self.g = f32(B, plane), f32(B, plane)
        self.pin = f32(B, env.Nx, env.Nz, 1, 1)
        self.x = f32(B, env.Nx, env.Nz, 1, 1).requires_grad_(True)                 # the persistent observer input: a leaf
        self.dy = f32(B, P, plane)
        self.start = torch.zeros((B, env.Nx, env.Nz), dtype=torch.float64, device=dev)
        self.losses = torch.zeros((self.epochs, B, len(F.ACTION_PARTS)), dtype=torch.float64, device=dev)
        self.ws = F.ctrl_action_workspace(B, P, plane, dev)
        self.unit = F.ctrl_policy_unit_stats(plane, dev)
        self.re_t = torch.full((B,), float(env.Re if self.re is None else self.re), dtype=torch.float32, device=dev)
        # the policy's optimizer as train_observer's full-field loop builds it: spectral-weight gradients written in place into
        # one flat bucket, the dead last-dim slices of the spectral weights skipped.  The dead-slice plan is made HERE (one
        # forward pass records the live extents) and not at the first step, so that state_tensors() names the final buffers
        self.bucket = FlatGradBucket(pm.parameters(), direct_module=pm)
        self.optimizer = FusedAdam(self.bucket, lr=self.lr, skip_dead_slices=True)
        self.optimizer.plan_dead_slices(self.pin, self.re_t)
        return self

    def state_tensors(self):
        """what a control iteration changes and the next one reads: the policy's parameters (one flat buffer) and Adam's
        moments.  (The step count is a host number that begin() resets.)  ControlLoop hands them to GraphedControlLoop, which
        restores them after its eager warm-up run, so the warm-up does not train the policy once too often."""
        opt = self.optimizer
        return [opt.flat_param, opt.exp_avg, opt.exp_avg_sq]

    def begin(self, p2):
        env = self.env
        d = env.detect_plane
        torch.neg(env.V[:, :, d, :], out=self.opV1)
        torch.neg(env.V[:, :, -d, :], out=self.start)
        F.ctrl_policy_begin(self.start, p2, self.a0, self.pin)
        self.optimizer.reset_state()

    def epoch(self, k):
        B, plane = self.env.B, self.env.Nx * self.env.Nz
        with torch.enable_grad():
            res = self.policy_model(self.pin, self.re_t)
            if res.numel() != B * plane:
                raise RuntimeError(f"PolicyObserverPolicy: the policy model returned {tuple(res.shape)} for {B} planes of {plane}")
            F.ctrl_policy_compose(self.a0, res.detach(), self.x, self.opV2)
            y = self.observer(self.x, self.re_t)
            if y.numel() != B * self.P * plane:
                raise RuntimeError(f"PolicyObserverPolicy: the observer returned {tuple(y.shape)} for {B} x {self.P} planes of {plane}")
            F.ctrl_policy_objective(y.detach(), self.x.detach(), reg=self.reg, parts=self.losses[k], dy=self.dy, ws=self.ws,
                                    unit=self.unit)
            (dx,) = torch.autograd.grad(y, self.x, self.dy.view(y.shape))
            F.ctrl_policy_grad(dx, self.x.detach(), self.losses[k], reg=self.reg, out=self.g)
            self.bucket.zero()
            torch.autograd.backward(res, self.g.view(res.shape))
        self.optimizer.step()
        self.res, self.dx = res.detach(), dx      # (for inspection: the last forward's correction and the observer's input gradient)

    def act(self, p2):
        self.begin(p2)
        for k in range(self.epochs):
            self.epoch(k)
        return self.opV1, self.opV2


def make_policy(policy_name, **kw):
    """the policy of a reference `policy_name` (run_control.py:135-226)"""
    if policy_name == "gt":
        return GtPolicy(kw.get("detect_plane"))
    if policy_name == "unmanipulated":
        return UnmanipulatedPolicy()
    if policy_name in ("fno", "rno"):
        cls = FnoPolicy if policy_name == "fno" else RnoPolicy
        return cls(kw["observer"], kw["p_norm"], kw["v_norm"], kw.get("zero_mean", False), kw.get("scale", 1.0), kw.get("clip", 0.0))
    if policy_name == "rand":
        raise NotImplementedError("policy `rand`: the reference's rand_control is a MATLAB call (compute_opposition)")
    if policy_name == "optimal-observer":
        if kw.get("observer") is None or kw.get("v_norm") is None:
            raise NotImplementedError("policy `optimal-observer` optimises the action through a trained full-field observer: pass "
                                      "observer=<a PINObserverFullField with in_dim = 1> and v_norm=<the wall-plane normaliser, "
                                      "FullFieldNSDataset.bound_v_norm> (run_control: model_name: PINObserverFullField, "
                                      "load_model_name and DATA_FOLDER of a full-field dataset); the bare name cannot build it")
        if int(kw.get("model_timestep", 1)) != 1:
            raise NotImplementedError(f"policy `optimal-observer` with model_timestep = {kw['model_timestep']}: it optimises one wall "
                                      "plane through an observer of one time step (model_timestep = 1)")
        opt = {k: kw[k] for k in ("epochs", "lr", "reg_weight", "re", "field_norm") if k in kw}
        return OptimalObserverPolicy(kw["observer"], kw["v_norm"], **opt)
    if policy_name == "optimal-policy-observer":
        if kw.get("policy_model") is None or kw.get("observer") is None:
            raise NotImplementedError("policy `optimal-policy-observer` trains a policy network through a trained full-field observer: "
                                      "pass policy_model=<a PolicyModel2D with in_dim = 1> and observer=<a PINObserverFullField with "
                                      "in_dim = 1> (run_control: model_name: PINObserverFullField, load_model_name and "
                                      "policy_model_name: PolicyModel2D); the bare name cannot build it")
        if int(kw.get("model_timestep", 1)) != 1:
            raise NotImplementedError(f"policy `optimal-policy-observer` with model_timestep = {kw['model_timestep']}: it trains on one "
                                      "wall plane through an observer of one time step (model_timestep = 1)")
        opt = {k: kw[k] for k in ("epochs", "lr", "reg_weight", "re") if k in kw}
        return PolicyObserverPolicy(kw["policy_model"], kw["observer"], **opt)
    raise RuntimeError("Not supported policy name.")


# ---------------------------------------------------------------------------------------------------------------------------
# the log
# ---------------------------------------------------------------------------------------------------------------------------
def check_log(rows, first=0, explode_at=EXPLODE_DIV):
    """the reference's `abs(reward_div()) > 10 -> "Control exploded!"` on host rows (n, B, 13) of the log, the first of them
    iteration `first`; raises naming the first offending iteration and environment (a non-finite divergence counts).
    explode_at=None: no check (sum(div) is the unweighted sum, so a state whose walls carry a net flux never has it small)"""
    if explode_at is None:
        return
    div = np.asarray(rows)[:, :, 0]
    bad = ~(np.abs(div) <= explode_at)
    if bad.any():
        t, b = np.argwhere(bad)[0]
        raise RuntimeError(f"Control exploded! iteration {first + int(t)}, environment {int(b)}: |sum(div)| = "
                           f"{abs(float(div[t, b])):.6g} > {explode_at:g}")


def infos_from_log(log, info_keys, init=None):
    """the reference's `info` dicts (step :639-664, cal_relative_info) from a host (T, B, 13) log: per iteration a list of B
    dicts; `init`: a list of B initial infos for the drag_reduction_relative keys (None: no relative keys)"""
    out = []
    for row in np.asarray(log):
        infos = []
        for b, r in enumerate(row):
            vals = (r[7], r[8], r[2], r[3], r[9], r[10], r[12], max(-abs(r[0]), -100.0), r[4] + r[5] + r[6])
            info = dict(zip(info_keys, (float(v) for v in vals)))
            if init is not None:
                info.update({k.replace("drag_reduction", "drag_reduction_relative"): info[k] / init[b][k]
                             for k in info_keys if "divergence" not in k})
            infos.append(info)
        out.append(infos)
    return out


class ControlResult:
    def __init__(self, log, infos, squeeze):
        self.log = log                                                 # (T, B, 13) numpy, columns functional.CONTROL_LOG
        self.infos = [i[0] for i in infos] if squeeze else infos       # one environment: a dict per iteration, as the reference


# ---------------------------------------------------------------------------------------------------------------------------
# dataset collection
# ---------------------------------------------------------------------------------------------------------------------------
def write_step(folder, i, arrays):
    """the six files of collected iteration i (run_control.py:234-293): float64, the reference's names, six-digit index"""
    idx = str(int(i)).zfill(6)
    for name in FIELDS:
        np.save(os.path.join(folder, f"{name}_{idx}.npy"), np.ascontiguousarray(arrays[name], dtype=np.float64))


def write_metadata(folder, re, stats, dpdx):
    """metadata.npy: re, per-field mean / std over the collected iterations below stats_steps, U_field.dpdx = every collected dPdx"""
    meta = {"re": re}
    for name in FIELDS:
        if name in stats:
            meta[name] = {"mean": np.asarray(stats[name][0]), "std": np.asarray(stats[name][1])}
    meta.setdefault("U_field", {})["dpdx"] = np.asarray(dpdx, dtype=np.float64)
    np.save(os.path.join(folder, "metadata.npy"), meta)


class Collector:
    """Writes the plane / full-field dataset of a rollout.  Per collected iteration i (i > collect_start): P_planes = the observed
    p2, V_planes = the applied opV2, U/V/W_field = the state before the step, du_dt = Fu of compute_rhs_py at the current dPdx.
    The running mean / M2 of the iterations with i < stats_steps stay on the device (functional.running_stats_update).  The
    snapshot of an iteration is staged in device buffers (inside the graph when the loop is graphed), copied to a small ring of
    pinned host buffers with an event per slot, and written by a worker thread, so the next iteration does not wait.
    B > 1: one sub-folder env_000... per environment; B = 1: the folder itself.  metadata.npy is written by finish()."""

    def __init__(self, folder, collect_start, stats_steps=100, re=-1, ring=3):
        self.folder, self.collect_start, self.stats_steps, self.re = folder, int(collect_start), int(stats_steps), re
        self.ring = max(int(ring), 2)
        self.count, self.collected, self.env = 0, [], None

    def wants(self, i):
        return i > self.collect_start

    def folders(self):
        B = self.env.B
        return [self.folder] if B == 1 else [os.path.join(self.folder, f"env_{b:03d}") for b in range(B)]

    def bind(self, env):
        self.env = env
        dev = env.device
        shapes = {"P_planes": (env.B, env.Nx, env.Nz), "V_planes": (env.B, env.Nx, env.Nz), "U_field": tuple(env.U.shape),
                  "V_field": tuple(env.V.shape), "W_field": tuple(env.W.shape), "du_dt": tuple(env.U.shape), "dpdx": (env.B,)}
        new = lambda shp, **kw: torch.zeros(shp, dtype=torch.float64, **kw)
        self.stage_bufs = {k: new(s, device=dev) for k, s in shapes.items()}
        self.mean = {k: new(shapes[k], device=dev) for k in FIELDS}
        self.m2 = {k: new(shapes[k], device=dev) for k in FIELDS}
        self.slots = [{k: new(s).pin_memory() for k, s in shapes.items()} for _ in range(self.ring)]
        self.events = [torch.cuda.Event() for _ in range(self.ring)]
        self.free = queue.Queue()
        for s in range(self.ring):
            self.free.put(s)
        for f in self.folders():
            os.makedirs(f, exist_ok=True)
        self.jobs, self.error, self.dpdx_rows = queue.Queue(), None, []
        self.worker = threading.Thread(target=self._write_loop, daemon=True)
        self.worker.start()
        return self

    def stage(self, p2, opV2):
        """device side, capturable: the snapshot of the state before the step, and du_dt at the current dPdx"""
        env, s = self.env, self.stage_bufs
        s["P_planes"].copy_(p2)
        s["V_planes"].copy_(opV2)
        s["U_field"].copy_(env.U)
        s["V_field"].copy_(env.V)
        s["W_field"].copy_(env.W)
        s["dpdx"].copy_(env.dPdx_dev)
        s["du_dt"].copy_(F.chanflow_rhs(env.grid, env.U, env.V, env.W, env.dPdx_dev)[0])

    def flush(self, i):
        """host side, eager: statistics, the copy into a pinned slot, the hand-over to the writer"""
        if self.error is not None:
            raise self.error
        s = self.stage_bufs
        if i < self.stats_steps:
            self.count += 1
            F.running_stats_update([s[k] for k in FIELDS], [self.mean[k] for k in FIELDS], [self.m2[k] for k in FIELDS], self.count)
        slot = self.free.get()                     # waits only when the writer is `ring` iterations behind
        for k, t in s.items():
            self.slots[slot][k].copy_(t, non_blocking=True)
        self.events[slot].record()
        self.collected.append(i)
        self.jobs.put((slot, i))

    def _write_loop(self):
        while True:
            job = self.jobs.get()
            if job is None:
                return
            slot, i = job
            try:
                self.events[slot].synchronize()
                host = self.slots[slot]
                for b, f in enumerate(self.folders()):
                    write_step(f, i, {k: host[k][b].numpy() for k in FIELDS})
                self.dpdx_rows.append(host["dpdx"].numpy().copy())
            except Exception as e:          # surfaces in the next flush() / finish()
                self.error = e
            finally:
                self.free.put(slot)

    def finish(self):
        """drain the writer and write metadata.npy; returns the folders"""
        self.jobs.put(None)
        self.worker.join()
        if self.error is not None:
            raise self.error
        n = max(self.count, 1)
        stats = {k: (self.mean[k].cpu().numpy(), torch.sqrt(self.m2[k] / n).cpu().numpy()) for k in FIELDS} if self.count else {}
        dpdx = np.stack(self.dpdx_rows) if self.dpdx_rows else np.zeros((0, self.env.B))
        for b, f in enumerate(self.folders()):
            write_metadata(f, self.re, {k: (m[b], s[b]) for k, (m, s) in stats.items()}, dpdx[:, b])
        return self.folders()


# ---------------------------------------------------------------------------------------------------------------------------
# the loop
# ---------------------------------------------------------------------------------------------------------------------------
class ControlLoop:
    """ControlLoop(env, policy, steps).run() -> ControlResult.  `env`: an eager ChannelFlowEnv (its state tensors are advanced
    in place); graph=True replays the whole iteration as one graph (functional.GraphedControlLoop), rebuilt when the
    environment's state tensors are replaced (load_state)."""

    def __init__(self, env, policy, steps, collector=None, graph=False, check_every=50, explode_at=EXPLODE_DIV):
        self.explode_at = explode_at
        dev = torch.device(getattr(env, "device", "cpu"))
        if dev.type != "cuda" or not torch.cuda.is_available():
            raise RuntimeError(f"fnoengine ControlLoop: the loop runs on the GPU (got device {dev}); the engine has no CPU path")
        if getattr(env, "_graph_wanted", False):
            raise RuntimeError("fnoengine ControlLoop: pass an eager environment (graph=False); the loop captures its own graph")
        if collector is not None and not policy.collects:
            collector = None                                                     # run_control.py:45-46
        self.env, self.policy, self.steps, self.collector = env, policy.bind(env), int(steps), collector
        self.graph_wanted, self.check_every = bool(graph), max(int(check_every), 1)
        shp = (env.B, env.Nx, env.Nz)
        self.p1 = torch.zeros(shp, dtype=torch.float64, device=dev)
        self.p2 = torch.zeros(shp, dtype=torch.float64, device=dev)
        self.row = torch.zeros((env.B, len(F.CONTROL_LOG)), dtype=torch.float64, device=dev)
        self.diag_ws = F.chanflow_diagnostics2_workspace(env.grid, env.B, dev)
        self.log = torch.zeros((self.steps, env.B, len(F.CONTROL_LOG)), dtype=torch.float64, device=dev)
        self.actions = self.observations = None      # run(keep_actions / keep_observations): (T, B, Nx, Nz) of opV2 / the observed p2
        self._graph = self._graph_of = None
        if collector is not None:
            collector.bind(env)

    def observe(self):
        env = self.env
        F.chanflow_wall_pressure(env.grid, env.poisson, env.U, env.V, env.W, env.dPdx_dev, ws=env.ws, out=(self.p1, self.p2))
        return self.p2

    def _iteration(self, out_row, stage):
        env = self.env
        opV1, opV2 = self.policy.act(self.p2)
        if stage:
            self.collector.stage(self.p2, opV2)
        F.chanflow_rk3_step(env.grid, env.poisson, env.U, env.V, env.W, opV1, opV2, env.dPdx_dev, env.meanU0, env.dt, ws=env.ws)
        F.chanflow_wall_pressure(env.grid, env.poisson, env.U, env.V, env.W, env.dPdx_dev, ws=env.ws, out=(self.p1, self.p2))
        F.chanflow_diagnostics2(env.grid, env.poisson, env.U, env.V, env.W, self.p2, env.dPdx_dev, out=out_row, ws=self.diag_ws)

    def _replay(self):
        env = self.env
        if self._graph is None or self._graph_of is not env.U:
            staged = self.collector is not None
            # (a policy that carries state from one iteration to the next names it: PolicyObserverPolicy.state_tensors)
            self._graph = F.GraphedControlLoop(lambda: self._iteration(self.row, staged),
                                               [env.U, env.V, env.W, env.dPdx_dev, self.p1, self.p2]
                                               + list(getattr(self.policy, "state_tensors", list)()), env.device)
            self._graph_of = env.U
        self._graph.replay()

    def run(self, keep_actions=False, keep_observations=False):
        env, col = self.env, self.collector
        self.observe()
        if keep_actions:
            self.actions = torch.zeros((self.steps,) + tuple(self.p2.shape), dtype=torch.float64, device=env.device)
        if keep_observations:
            self.observations = torch.zeros((self.steps,) + tuple(self.p2.shape), dtype=torch.float64, device=env.device)
        checked = 0
        for i in range(self.steps):
            if i == 0 and isinstance(self.policy, UnmanipulatedPolicy):
                env.reset_init()
            collect = col is not None and col.wants(i)
            if keep_observations:
                self.observations[i].copy_(self.p2)
            if self.graph_wanted:
                self._replay()
                self.log[i].copy_(self.row)
            else:
                self._iteration(self.log[i], collect)
            if keep_actions:
                self.actions[i].copy_(self.policy.opV2)
            if collect:
                col.flush(i)
            if (i + 1) % self.check_every == 0:
                check_log(self.log[checked:i + 1].cpu().numpy(), checked, self.explode_at)
                checked = i + 1
        log = self.log.cpu().numpy()
        if col is not None:
            col.finish()
        check_log(log[checked:], checked, self.explode_at)
        init = env.info_init
        if init is not None:
            init = [init] if env._squeeze else init
        elif self.steps:
            init = infos_from_log(log[:1], env.INFO_KEYS)[0]       # after reset_init: relative to the first iteration
        return ControlResult(log, infos_from_log(log, env.INFO_KEYS, init), env._squeeze)
