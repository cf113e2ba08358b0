"""PINO residual losses with the reference surface (libs/pino_utils/losses.py): the FDM-in-time / spectral-in-space
Navier-Stokes vorticity residual and the two relative-L2 terms the fine-tuning loop (train_pino.py:98-101) combines
(:68-104, 246-262, 288-291), the Burgers residual and its two mean-square terms (:200-243: FDM_Burgers, PINO_loss), the Darcy
residual and its relative-L2 term (:6-65: FDM_Darcy, darcy_loss) and the relative L2 data loss (:151-197: LpLoss).  The
arithmetic runs in the HIP engine (functional.pino_loss, burgers_loss, burgers_residual, darcy_loss, darcy_residual,
lp_loss_rel); there is no CPU path."""
import math

import torch

from ... import functional as F


def get_forcing(S):
    """-4 cos(4 y) on the periodic grid y_j = 2 pi j / S, shape (1, S, S, 1)  (losses.py:288-291)."""
    y = torch.arange(S, dtype=torch.float32) * (2 * math.pi / S)
    return (-4 * torch.cos(4 * y)).reshape(1, 1, S, 1).repeat(1, S, 1, 1)


def PINO_loss3d(u, u0, forcing, v=1 / 40, t_interval=1.0):
    """(loss_ic, loss_f): LpLoss(size_average=True) of u[..., 0] vs u0 and of the residual vs the forcing."""
    B, nx, ny, nt = u.size(0), u.size(1), u.size(2), u.size(3)
    u = u.reshape(B, nx, ny, nt)
    if not torch.is_tensor(v):
        v = torch.full((B,), float(v), dtype=torch.float32, device=u.device)
    return F.pino_loss(u, u0.reshape(B, nx, ny), forcing.to(u.device), v.reshape(B).to(u.device), t_interval)


Channelflow_PINO_loss = PINO_loss3d      # libs/envs/diff_control_env.py:44-60 is the same computation


class LpLoss(object):
    """Relative L2 loss (losses.py:151-197).  `rel` / `__call__` run on functional.lp_loss_rel; what the engine has no kernel
    for - `abs`, p != 2, reduction=False - raises NotImplementedError naming the option."""

    def __init__(self, d=2, p=2, size_average=True, reduction=True):
        assert d > 0 and p > 0
        if p != 2:
            raise NotImplementedError(f"LpLoss: p={p} (the engine's loss is the relative L2 norm, p=2)")
        if not reduction:
            raise NotImplementedError("LpLoss: reduction=False (per-sample norms are not returned by the engine)")
        self.d, self.p, self.reduction, self.size_average = d, p, reduction, size_average

    def abs(self, x, y):
        raise NotImplementedError("LpLoss: abs (only the relative norm `rel` runs on the engine)")

    def rel(self, x, y):
        return F.lp_loss_rel(x, y, size_average=self.size_average)

    def __call__(self, x, y):
        return self.rel(x, y)


def FDM_Burgers(u, v, D=1):
    """Du (B, nt - 2, nx) of u (B, nt, nx[, 1]): central difference in t, spectral derivatives in x, unit domain
    (losses.py:200-220).  Not differentiable; PINO_loss is what training differentiates."""
    if D != 1:
        raise NotImplementedError(f"FDM_Burgers: D={D} (the engine's kernel is built for the unit domain, D=1)")
    return F.burgers_residual(u.reshape(u.size(0), u.size(1), u.size(2)), float(v))


def PINO_loss(u, u0, v):
    """(loss_u, loss_f): mean squares of u[:, 0] - u0 and of the Burgers residual (losses.py:223-243)."""
    return F.burgers_loss(u.reshape(u.size(0), u.size(1), u.size(2)), u0, float(v))


def FDM_Darcy(u, a, D=1):
    """Du (B, S - 4, S - 4) = -div(a grad u) of u, a (B, S, S[, 1]) by two central differences on the unit square
    (losses.py:6-36).  Not differentiable; darcy_loss is what training differentiates."""
    if D != 1:
        raise NotImplementedError(f"FDM_Darcy: D={D} (the engine's kernel is built for the unit domain, D=1)")
    B, S = u.size(0), u.size(1)
    return F.darcy_residual(u.reshape(B, S, S), a.reshape(B, S, S))


def darcy_loss(u, a):
    """LpLoss(size_average=True).rel of the Darcy residual against ones (losses.py:39-65).  functional.darcy_loss also
    takes the mollifier and the data target, which the training loop passes for one fused call."""
    B, S = u.size(0), u.size(1)
    return F.darcy_loss(u.reshape(B, S, S), a.reshape(B, S, S))
