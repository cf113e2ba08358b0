"""What the optimal-observer policy (control.OptimalObserverPolicy, csrc/k_action_opt.h) is held to: the fixture, the float64
and the reference-dtype restatements of run_control.py:186-224, the closed forms the kernels evaluate, the comparison and the
error log.  A helper module, not a conftest; shared by tests/test_action_opt_host.py (CPU) and tests/test_action_opt_gpu.py.

Comparison (tests/judging.py::accept, judge_budget):  err_engine == 0 or err_engine < max(floor, BUDGET_SLACK * err_ref32),
err = relative L2 against the float64 restatement, err_ref32 = the error of the reference-dtype restatement (float32 observer
through oracle.observers_oracle, torch autograd, torch.optim.Adam) on the same inputs.  Floor 1e-5 (the project's TOL_G) for
the loss, the input gradient and the displacement; none for the elementwise kernels.  Every figure goes to
profiles/r16_action_opt_errors.txt, one block per case, before anything is asserted.

Why the displacement and never the final action: ten Adam steps of 1e-3 move an action of magnitude 0.3 by 3 %; an error of
the whole update would hide behind the start action.  Why reg = 0 as well as 0.1: with default-initialised weights the
regulariser carries |g| = 0.1 against 8.5e-4 from the observer; at 0.1 an error of the observer's input gradient would hide.
Adam's first step is lr * sign(g), so the fixture is valid only while no |g_i| is within reach of the float32 error
(`sign_margin`), a condition on the inputs that the host test checks before the GPU is asked anything."""
import functools
import math
import os

import numpy as np
import torch

from oracle import observers_oracle as OO
from tests.judging import TOL_G, SectionLog, judge_budget, rejected, rel_err  # noqa: F401  (re-exported to the tests)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOG = SectionLog(os.path.join(ROOT, "profiles", "r16_action_opt_errors.txt"))
log_block = LOG.replace
judge = functools.partial(judge_budget, LOG)        # rows: (name, err_engine, err_ref32, floor)
FLOOR = TOL_G
EPS, RE, LR, BETAS, ADAM_EPS, EPOCHS = 1e-5, 180.0, 1e-3, (0.9, 0.999), 1e-8, 10
NX = NZ = 32
PLANES, LAYERS, MODES, PAD, FC_DIM = 3, [64] * 5, [(4, 4, 4)] * 4, [0.0, 0.0625], 128


# ---------------------------------------------------------------------------------------------------------------------------
# fixture
# ---------------------------------------------------------------------------------------------------------------------------
def observer(modes=4):
    """PINObserverFullField of tests/test_parity_gpu.py:578 under torch.manual_seed(0), on the CPU"""
    from pde_policylearning_amd.libs.models.pino_models import PINObserverFullField
    torch.manual_seed(0)
    return PINObserverFullField(plane_num=PLANES, modes1=[modes] * 4, modes2=[modes] * 4, modes3=[modes] * 4, fc_dim=FC_DIM,
                                layers=list(LAYERS), in_dim=1, out_dim=1, act="gelu", pad_ratio=list(PAD))


def params_of(model, dtype=None):
    """the module's parameters for the oracle, on the CPU; dtype float64: cast (complex weights to complex128)"""
    out = {}
    for k, v in model.state_dict().items():
        v = v.detach().cpu().clone()
        if dtype == torch.float64:
            v = v.to(torch.complex128 if v.is_complex() else torch.float64)
        out[k] = v
    return out


class Norm:
    """what the policy reads of a NormalizerGivenMeanStd"""

    def __init__(self, mean, std, eps=EPS):
        self.mean, self.std, self.eps = np.asarray(mean, dtype=np.float64), np.asarray(std, dtype=np.float64), eps


def stats(nx=NX, nz=NZ, seed=3):
    """float64 wall-plane statistics: mean = 0.05 N(0, 1), std = 0.2 + 0.1 U(0, 1)"""
    g = torch.Generator().manual_seed(seed)
    mean = 0.05 * torch.randn(nx, nz, generator=g, dtype=torch.float64)
    std = 0.2 + 0.1 * torch.rand(nx, nz, generator=g, dtype=torch.float64)
    return mean, std


def start_action(B=1, nx=NX, nz=NZ, seed=5):
    """(B, nx, nz) float64: 0.3 N(0, 1)"""
    g = torch.Generator().manual_seed(seed)
    return 0.3 * torch.randn(B, nx, nz, generator=g, dtype=torch.float64)


def forward(p, x, re):
    """the oracle's PINObserverFullField on x (B, Nx, Nz, 1, 1) -> (B, P, Nx, Nz, 1), in the dtype of p and x"""
    re = torch.as_tensor(re, dtype=x.dtype).reshape(-1).expand(x.shape[0])
    return OO.pinobserver_fullfield_forward(p, x, re, LAYERS, MODES, PAD)


# ---------------------------------------------------------------------------------------------------------------------------
# the reference's expressions under torch autograd and torch.optim.Adam (one environment)
# ---------------------------------------------------------------------------------------------------------------------------
def reference_loss(p, a, mean, std, re, reg, ref32):
    """run_control.py:211-220 on the leaf `a` (Nx, Nz).  ref32: the reference's dtypes - a float32 leaf, encoded against float64
    statistics and rounded with .float(), a float32 observer, planes decoded against the float64 statistics, torch.norm of
    the float64 field plus reg * torch.norm of the float32 leaf.  Otherwise float64 throughout.  -> loss, y (graph attached)"""
    S = std + EPS
    x = (a - mean) / S
    if ref32:
        x = x.float()
    y = forward(p, x[None, :, :, None, None], re)
    field = torch.stack([y[:, k, :, :, 0] * S + mean for k in range(y.shape[1])], dim=2)
    return torch.norm(field) + reg * torch.norm(a), y


def policy_torch(p, a0, mean, std, re, reg, epochs, ref32):
    """the inner loop with torch.optim.Adam from a = float32(a0) (held in float64 when not ref32).  -> dict of float64:
    start, a (final), disp, loss (epochs,), g (epochs, Nx, Nz) the gradients Adam was given, opV2 (final minus its mean)"""
    dt = torch.float32 if ref32 else torch.float64
    start = a0.detach().float()
    a = start.to(dt).clone().requires_grad_(True)
    opt = torch.optim.Adam([a], lr=LR, betas=BETAS, eps=ADAM_EPS)
    loss, gs = [], []
    for _ in range(epochs):
        opt.zero_grad()
        L, _ = reference_loss(p, a, mean, std, re, reg, ref32)
        L.backward()
        loss.append(float(L.detach()))
        gs.append(a.grad.detach().double().clone())
        opt.step()
    fin = a.detach().double()
    return {"start": start.double(), "a": fin, "disp": fin - start.double(), "loss": torch.tensor(loss, dtype=torch.float64),
            "g": torch.stack(gs), "opV2": fin - fin.mean()}


# ---------------------------------------------------------------------------------------------------------------------------
# the closed forms the kernels evaluate (ISSUE "Semantics to reproduce")
# ---------------------------------------------------------------------------------------------------------------------------
def objective_closed(y, a, mean, std, reg, drop_S=False):
    """y (P, Nx, Nz), a (Nx, Nz) -> (loss, nf, na) float64 scalars and dy float64 (P, Nx, Nz) = field / nf * S, 0 where nf == 0.
    drop_S: the planted fault - dy = field / nf."""
    S = std + EPS
    field = y.double() * S + mean
    nf, na = torch.sqrt((field * field).sum()), torch.sqrt((a.double() ** 2).sum())
    dy = torch.zeros_like(field) if float(nf) == 0.0 else field / nf * (1.0 if drop_S else S)
    return nf + reg * na, nf, na, dy


def g_closed(dx, a, std, reg, na, na_squared=False):
    """g = dx / S + reg * a / na in float64 (second term 0 where na == 0).  na_squared: the planted fault - a / na^2."""
    S = std + EPS
    second = torch.zeros_like(S) if float(na) == 0.0 else reg * a.double() / (na * na if na_squared else na)
    return dx.double() / S + second


def adam_scalars(step):
    """{step_size, sqrt(bias correction 2)} formed in double and rounded once (fno_adam_scalars)"""
    f32 = lambda v: torch.tensor(v, dtype=torch.float32)      # noqa: E731
    return f32(LR / (1.0 - BETAS[0] ** step)), f32(math.sqrt(1.0 - BETAS[1] ** step))


def policy_restated(p, a0, mean, std, re, reg, epochs, drop_S=False, na_squared=False, bias_step_shift=0):
    """k_action_opt.h's arithmetic in torch on the CPU: the float32 leaf, x rounded once, the float32 oracle observer and its
    autograd backward given dy, g assembled in float64 and rounded once, k_adam's float32 step without the fused
    multiply-adds.  The three keyword arguments plant a fault each (bias_step_shift = -1: the bias corrections of the step
    before, from the second step on).  -> as policy_torch"""
    f32 = lambda v: torch.tensor(v, dtype=torch.float32)      # noqa: E731
    S = std + EPS
    start = a0.detach().float()
    a, m, v = start.clone(), torch.zeros_like(start), torch.zeros_like(start)
    loss, gs = [], []
    for k in range(epochs):
        x = ((a.double() - mean) / S).float().requires_grad_(True)
        y = forward(p, x[None, :, :, None, None], re)
        L, nf, na, dy = objective_closed(y.detach()[0, :, :, :, 0], a, mean, std, reg, drop_S)
        (dx,) = torch.autograd.grad(y, x, dy.float()[None, :, :, :, None])
        g = g_closed(dx, a, std, reg, na, na_squared).float()
        step_size, bc2_sqrt = adam_scalars(max(k + 1 + bias_step_shift, 1))
        m = m + (g - m) * f32(1.0 - BETAS[0])
        v = f32(BETAS[1]) * v + (g * g) * f32(1.0 - BETAS[1])
        a = a - step_size * (m / (torch.sqrt(v) / bc2_sqrt + f32(ADAM_EPS)))
        loss.append(float(L))
        gs.append(g.double())
    fin = a.double()
    return {"start": start.double(), "a": fin, "disp": fin - start.double(), "loss": torch.tensor(loss, dtype=torch.float64),
            "g": torch.stack(gs), "opV2": fin - fin.mean()}


def sign_margin(g32, g64):
    """(min |g| / max |g| of the float64 gradient, max |g32 - g64| / max |g64|): the fixture needs the first >= 20 x the second"""
    top = float(g64.abs().max())
    return float(g64.abs().min()) / top, float((g32 - g64).abs().max()) / top


def policy_rows(tag, got, ref32, ref64):
    """rows for judge(): displacement, per-epoch loss and final opV2 of `got` against the float64 restatement"""
    rows = [(f"{tag} displacement", rel_err(got["disp"], ref64["disp"]), rel_err(ref32["disp"], ref64["disp"]), FLOOR),
            (f"{tag} loss per epoch", rel_err(got["loss"], ref64["loss"]), rel_err(ref32["loss"], ref64["loss"]), FLOOR)]
    if "g" in got:
        rows.append((f"{tag} gradient epoch 0", rel_err(got["g"][0], ref64["g"][0]), rel_err(ref32["g"][0], ref64["g"][0]), FLOOR))
    # opV2 = final - its mean: compared as the displacement of the zero-mean action from the zero-mean start, for the reason
    # the displacement is (module docstring)
    z = lambda r: r["opV2"] - (r["start"] - r["start"].mean())      # noqa: E731
    rows.append((f"{tag} opV2 - zero-mean start", rel_err(z(got), z(ref64)), rel_err(z(ref32), z(ref64)), FLOOR))
    return rows


# ---------------------------------------------------------------------------------------------------------------------------
# the workgroup's fixed-order sum (k_chanflow_step.h cf_block_sum) restated, for the bit-for-bit plane mean of k_act_finish
# ---------------------------------------------------------------------------------------------------------------------------
def block_sum_256(v):
    """v: float64 numpy array; thread t adds elements t, t + 256, ... in order, the 64 lanes of a wave combine by the xor
    butterfly 32, 16, ..., 1, the four waves as (w0 + w1) + (w2 + w3)"""
    v = np.asarray(v, dtype=np.float64).ravel()
    acc = np.zeros(256)
    for s in range(0, v.size, 256):
        part = v[s:s + 256]
        acc[:part.size] = acc[:part.size] + part
    w = acc.reshape(4, 64)
    lane = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        w = w + w[:, lane ^ off]
    return (w[0, 0] + w[1, 0]) + (w[2, 0] + w[3, 0])
