"""Fused training losses: relative Lp, the PINO / Burgers / Darcy residual losses, the neuralop Sobolev (H1) and Hs losses.
"""
import ctypes as C
import functools
import math

import torch

from .. import _lib
from ._core import _bytes, _call, _operand, _refuse, _require_cuda, STREAM


def _grad_scalar(entry, name, g, anchor):
    """an incoming gradient of a scalar loss as one float32 element the backward kernels read on the device"""
    return _operand(entry, name, g.contiguous().to(torch.float32), anchor, numel=1).reshape(1)


def _drop_unit_channel(t):
    """a trailing singleton channel is dropped (a model's output is (..., 1))"""
    return t[..., 0] if t.dim() == 4 and t.shape[-1] == 1 else t


# ----------------------------------------------------------------------------
# training-step tail: decode + relative-L2 loss (Adam on a flat bucket: optim.py)
# ----------------------------------------------------------------------------
class _LpLossRelFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target, mean, std, eps, size_average):
        e = "lp_loss_rel"
        _require_cuda(pred, "pred")
        _require_cuda(target, "target")
        B = pred.shape[0]
        pred_c = pred.contiguous()
        n = pred_c.numel() // B
        if target.numel() != pred_c.numel():
            raise RuntimeError(f"fnoengine {e}: pred {tuple(pred.shape)} vs target {tuple(target.shape)}")
        tgt_c = _operand(e, "target", target, pred)
        mean_c = _operand(e, "mean", mean, pred, optional=True)
        std_c = _operand(e, "std", std, pred, optional=True)
        if mean_c is not None and std_c is not None and mean_c.numel() != std_c.numel():
            raise RuntimeError(f"fnoengine {e}: mean and std must have the same number of elements")
        stat_len = std_c.numel() if std_c is not None else mean_c.numel() if mean_c is not None else 1
        nws = _lib.lib().fno_lploss_workspace_bytes(B)
        ws = _bytes(nws, pred.device)
        loss = torch.empty((), dtype=torch.float32, device=pred.device)
        _call("lploss_rel_forward", pred.device, "fno_lploss_rel_forward", B, n, pred_c, tgt_c, mean_c, std_c, stat_len,
              float(eps), int(bool(size_average)), loss, ws, nws, STREAM)
        ctx.save_for_backward(pred_c, tgt_c, std_c if std_c is not None else pred_c.new_empty(0), ws)
        ctx.meta = (B, n, stat_len, float(eps), std_c is not None, nws, pred.shape)
        return loss

    @staticmethod
    def backward(ctx, gloss):
        pred_c, tgt_c, std_c, ws = ctx.saved_tensors
        B, n, stat_len, eps, has_std, nws, shape = ctx.meta
        dpred = torch.empty_like(pred_c)
        g = _operand("lp_loss_rel backward", "gloss", gloss.contiguous().to(torch.float32), pred_c, numel=1)
        _call("lploss_rel_backward", pred_c.device, "fno_lploss_rel_backward", B, n, pred_c, tgt_c, std_c if has_std else None,
              stat_len, eps, g, dpred, ws, nws, STREAM)
        return dpred.view(shape), None, None, None, None, None


def lp_loss_rel(pred, target, mean=None, std=None, eps=1e-5, size_average=False):
    """LpLoss(d=2, p=2).rel of the DECODED fields in two streaming passes (libs/utilities3.py:115-129,
    323-334; run_pde_observers.py:188-192).  mean / std: None (no decode), scalars or per-element planes
    broadcast over the batch."""
    return _LpLossRelFn.apply(pred, target, mean, std, eps, size_average)


# ----------------------------------------------------------------------------
# PINO residual loss (spectral Navier-Stokes vorticity residual + initial condition)
# ----------------------------------------------------------------------------
class _PinoLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, u, u0, forcing, visc, t_interval):
        e = "pino_loss"
        _require_cuda(u, "u")
        B, n, n2, nt = u.shape
        if n != n2:
            raise RuntimeError(f"fnoengine {e}: square grids only (got {n} x {n2})")
        u_c = u.contiguous()
        u0_c = _operand(e, "u0", u0, u, numel=B * n * n).reshape(B, n, n)
        f_c = _operand(e, "forcing", forcing, u, numel=n * n).reshape(n, n)
        v_c = _operand(e, "visc", visc, u, numel=B).reshape(B)
        nws = _lib.lib().fno_pino_loss_workspace_bytes(B, n, nt)
        ws = _bytes(nws, u.device)
        losses = torch.empty(2, dtype=torch.float32, device=u.device)
        _call("pino_loss_forward", u.device, "fno_pino_loss_forward", B, n, nt, u_c, u0_c, f_c, v_c, float(t_interval),
              losses[0:1], losses[1:2], ws, nws, STREAM)
        ctx.save_for_backward(u_c, u0_c, f_c, v_c, ws)
        ctx.meta = (B, n, nt, float(t_interval), nws, u.shape)
        return losses[0], losses[1]

    @staticmethod
    def backward(ctx, g_ic, g_f):
        u_c, u0_c, f_c, v_c, ws = ctx.saved_tensors
        B, n, nt, t_interval, nws, shape = ctx.meta
        du = torch.empty_like(u_c)
        gi = _grad_scalar("pino_loss backward", "g_ic", g_ic, u_c)
        gf = _grad_scalar("pino_loss backward", "g_f", g_f, u_c)
        _call("pino_loss_backward", du.device, "fno_pino_loss_backward", B, n, nt, u_c, u0_c, f_c, v_c, t_interval, gi, gf, du,
              ws, nws, STREAM)
        return du.view(shape), None, None, None, None


def pino_loss(u, u0, forcing, visc, t_interval=1.0):
    """(loss_ic, loss_f) of Channelflow_PINO_loss / PINO_loss3d (libs/envs/diff_control_env.py:44-60):
    u (B, n, n, nt) model output, u0 (B, n, n), forcing (n, n) or (1, n, n, 1), visc (B,) = 1 / Re.
    Differentiable w.r.t. u.  n in {32, 64, 128} (one workgroup per plane, in-LDS FFTs) or 256 (row / column / row
    slab passes through HBM)."""
    return _PinoLossFn.apply(u, u0, forcing, visc, t_interval)


# ----------------------------------------------------------------------------
# Burgers residual loss (FDM_Burgers + PINO_loss, libs/pino_utils/losses.py:200-243)
# ----------------------------------------------------------------------------
BURGERS_NX = (32, 64, 128)


def _burgers_rows(e, u):
    """u as (B, nt, nx): a trailing singleton channel is dropped (the model's output is (B, nt, nx, 1))"""
    u = _drop_unit_channel(u)
    if u.dim() != 3:
        raise RuntimeError(f"fnoengine {e}: `u` must be (B, nt, nx) or (B, nt, nx, 1) (got {tuple(u.shape)})")
    return u


def burgers_loss_supported(u):
    """the shapes k_burgers_loss.h takes: float32 on the GPU, (B, nt, nx[, 1]) with nt >= 3 and nx in BURGERS_NX"""
    u = _drop_unit_channel(u)
    return bool(u.is_cuda and u.dtype == torch.float32 and u.dim() == 3 and u.shape[0] >= 1 and u.shape[1] >= 3
                and u.shape[2] in BURGERS_NX)


def _burgers_forward(e, u, u0, visc):
    """(u_c, u0_c, losses (2,), ws, nws) of one forward call; `u0` None: the initial-condition term is taken against u[:, 0]"""
    _require_cuda(u, "u")
    u_c = _burgers_rows(e, u).contiguous()
    B, nt, nx = u_c.shape
    u0_c = u_c[:, 0].contiguous() if u0 is None else _operand(e, "u0", u0, u, numel=B * nx).reshape(B, nx)
    nws = _lib.lib().fno_burgers_loss_workspace_bytes(B, nt, nx)
    ws = _bytes(nws, u.device)
    losses = torch.empty(2, dtype=torch.float32, device=u.device)
    _call("burgers_loss_forward", u.device, "fno_burgers_loss_forward", B, nt, nx, u_c, u0_c, float(visc), losses[0:1],
          losses[1:2], ws, nws, STREAM)
    return u_c, u0_c, losses, ws, nws


class _BurgersLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, u, u0, visc):
        u_c, u0_c, losses, ws, nws = _burgers_forward("burgers_loss", u, u0, visc)
        ctx.save_for_backward(u_c, u0_c, ws)
        ctx.meta = (float(visc), nws, u.shape)
        return losses[0], losses[1]

    @staticmethod
    def backward(ctx, g_u, g_f):
        u_c, u0_c, ws = ctx.saved_tensors
        visc, nws, shape = ctx.meta
        B, nt, nx = u_c.shape
        du = torch.empty_like(u_c)
        gu = _grad_scalar("burgers_loss backward", "g_u", g_u, u_c)
        gf = _grad_scalar("burgers_loss backward", "g_f", g_f, u_c)
        _call("burgers_loss_backward", du.device, "fno_burgers_loss_backward", B, nt, nx, u_c, u0_c, visc, gu, gf, du, ws, nws,
              STREAM)
        return du.view(shape), None, None


def burgers_loss(u, u0, visc):
    """(loss_u, loss_f) of PINO_loss (libs/pino_utils/losses.py:223-243): u (B, nt, nx) or (B, nt, nx, 1) model output,
    u0 (B, nx) initial condition, visc a host float; domain length 1.  Differentiable w.r.t. u.  nx in {32, 64, 128}."""
    return _BurgersLossFn.apply(u, u0, visc)


def burgers_residual(u, visc):
    """Du (B, nt - 2, nx) of FDM_Burgers (libs/pino_utils/losses.py:200-220) as the forward kernel of burgers_loss stores
    it: the first array of its workspace (fno_abi.hip carve_burgers).  Not differentiable."""
    u_c, _, _, ws, _ = _burgers_forward("burgers_residual", u.detach(), None, visc)
    B, nt, nx = u_c.shape
    return ws[:4 * B * (nt - 2) * nx].view(torch.float32).reshape(B, nt - 2, nx)


# ----------------------------------------------------------------------------
# Darcy residual loss (FDM_Darcy + darcy_loss, libs/pino_utils/losses.py:6-65; mollifier and data term of train_2d.py:58-82)
# ----------------------------------------------------------------------------
DARCY_S_MIN, DARCY_S_MAX = 5, 4096           # csrc/k_darcy_loss.h DARCY_SMAX


def _darcy_plane(e, name, t):
    """t as (B, S, S): a trailing singleton channel is dropped (the model's output is (B, S, S, 1))"""
    t = _drop_unit_channel(t)
    if t.dim() != 3 or t.shape[1] != t.shape[2]:
        raise RuntimeError(f"fnoengine {e}: `{name}` must be (B, S, S) or (B, S, S, 1) on a square grid (got {tuple(t.shape)})")
    return t


def darcy_loss_supported(u):
    """the shapes k_darcy_loss.h takes: float32 on the GPU, (B, S, S[, 1]) with DARCY_S_MIN <= S <= DARCY_S_MAX"""
    u = _drop_unit_channel(u)
    return bool(u.is_cuda and u.dtype == torch.float32 and u.dim() == 3 and u.shape[0] >= 1 and u.shape[1] == u.shape[2]
                and DARCY_S_MIN <= u.shape[1] <= DARCY_S_MAX)


def _darcy_forward(e, u, a, y, mollifier):
    """(u_c, a_c, y_c, mol_c, losses (2,): data, f, ws, nws) of one forward call"""
    _require_cuda(u, "u")
    u_c = _darcy_plane(e, "u", u).contiguous()
    B, S, _ = u_c.shape
    a_c = _operand(e, "a", _darcy_plane(e, "a", a), u, shape=u_c.shape)
    y_c = None if y is None else _operand(e, "y", y, u, numel=B * S * S).reshape(B, S, S)
    mol_c = None if mollifier is None else _operand(e, "mollifier", mollifier, u, numel=S * S).reshape(S, S)
    nws = _lib.lib().fno_darcy_loss_workspace_bytes(B, S)
    ws = _bytes(nws, u.device)
    losses = torch.empty(2, dtype=torch.float32, device=u.device)
    _call("darcy_loss_forward", u.device, "fno_darcy_loss_forward", B, S, u_c, mol_c, a_c, y_c,
          None if y_c is None else losses[0:1], losses[1:2], ws, nws, STREAM)
    return u_c, a_c, y_c, mol_c, losses, ws, nws


class _DarcyLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, u, a, y, mollifier):
        u_c, a_c, y_c, mol_c, losses, ws, nws = _darcy_forward("darcy_loss", u, a, y, mollifier)
        empty = u_c.new_empty(0)
        ctx.save_for_backward(u_c, a_c, empty if y_c is None else y_c, empty if mol_c is None else mol_c, ws)
        ctx.meta = (y_c is not None, mol_c is not None, nws, u.shape)
        return losses[0], losses[1]                  # without y, losses[0] is never written and darcy_loss drops it

    @staticmethod
    def backward(ctx, g_data, g_f):
        u_c, a_c, y_c, mol_c, ws = ctx.saved_tensors
        has_y, has_mol, nws, shape = ctx.meta
        B, S, _ = u_c.shape
        dout = torch.empty_like(u_c)
        e = "darcy_loss backward"
        gd = _grad_scalar(e, "g_data", g_data, u_c) if has_y else None
        gf = _grad_scalar(e, "g_f", g_f, u_c)
        _call("darcy_loss_backward", dout.device, "fno_darcy_loss_backward", B, S, u_c, mol_c if has_mol else None, a_c,
              y_c if has_y else None, gd, gf, dout, ws, nws, STREAM)
        return dout.view(shape), None, None, None


def darcy_loss(u, a, y=None, mollifier=None):
    """loss_f, or (loss_data, loss_f) when `y` is given: darcy_loss (libs/pino_utils/losses.py:39-65) of pred = u * mollifier
    and LpLoss(size_average=True)(pred, y) (train_2d.py:75-82) in one fused call.  u (B, S, S) or (B, S, S, 1) model output,
    a (B, S, S) coefficient (data: no gradient; `x[..., 0]`, non-contiguous, is copied), y (B, S, S) solution, mollifier
    (S, S); any S from 5 up.  Differentiable w.r.t. u.  A sample whose residual norm ||Du_b - 1|| is exactly zero contributes
    a zero gradient (the reference's autograd gives NaN there)."""
    loss_data, loss_f = _DarcyLossFn.apply(u, a, y, mollifier)
    return loss_f if y is None else (loss_data, loss_f)


def darcy_residual(u, a, mollifier=None):
    """Du (B, S - 4, S - 4) of FDM_Darcy (libs/pino_utils/losses.py:6-36) on u * mollifier as the forward kernel of
    darcy_loss stores it: the first array of its workspace (fno_abi.hip carve_darcy).  Not differentiable."""
    u_c, _, _, _, _, ws, _ = _darcy_forward("darcy_residual", u.detach(), a, None, mollifier)
    B, S, _ = u_c.shape
    return ws[:4 * B * (S - 4) * (S - 4)].view(torch.float32).reshape(B, S - 4, S - 4)


# ----------------------------------------------------------------------------
# Sobolev (H1) and L2 training losses of neuralop (LpLoss p = 2, H1Loss: neuralop/training/losses.py:62-277)
# ----------------------------------------------------------------------------
SOBOLEV_REDUCE = {None: 0, "sum": 1, "mean": 2}        # csrc/k_sobolev_loss.h SOB_REDUCE_*


def sobolev_loss_supported(x, d):
    """what k_sobolev_loss.h takes: float32 on the GPU, 1 <= d <= 3 trailing grid axes of extent >= 2 each, at least one
    plane, a plane of fewer than 2^31 elements"""
    return bool(isinstance(d, int) and 1 <= d <= 3 and x.is_cuda and x.dtype == torch.float32 and x.dim() >= d
                and all(n >= 2 for n in x.shape[x.dim() - d:]) and math.prod(x.shape[:x.dim() - d]) >= 1
                and math.prod(x.shape[x.dim() - d:]) < 2 ** 31)


@functools.lru_cache(maxsize=256)
def _sobolev_plan(shape, d, h, order, relative, fix, reduce, squeeze):
    """The host's part of one configuration, worked out once: (the scalar arguments of both entry points, workspace bytes,
    planes, channels, shape of the result).  The step factors are float64 here and rounded once by the library."""
    e = "sobolev_loss"
    if not isinstance(d, int) or not 1 <= d <= 3 or len(shape) < d:
        raise _refuse(e, "d", "count 1, 2 or 3 trailing grid axes of `x`", f"d={d}, x of shape {tuple(shape)}")
    if reduce not in SOBOLEV_REDUCE:
        raise _refuse(e, "reduce", "be None, 'sum' or 'mean'", repr(reduce))
    if len(h) != d or len(fix) != d:
        raise _refuse(e, "h, fix", f"have one entry per grid axis (d={d})", f"h={list(h)}, fix={list(fix)}")
    lead, grid = shape[:len(shape) - d], shape[len(shape) - d:]
    if reduce is not None and len(lead) < 1:
        raise _refuse(e, "reduce", "be None for an input without a leading axis", repr(reduce))
    planes = math.prod(lead)
    channels = planes // lead[0] if reduce is not None and lead[0] > 0 else 1
    dims = (C.c_int * 3)(*grid)
    hs = [float(v) for v in h]
    inv2h, invh = (C.c_double * 3)(*[1.0 / (2.0 * v) for v in hs]), (C.c_double * 3)(*[1.0 / v for v in hs])
    mask = sum(1 << k for k, f in enumerate(fix) if f)
    scal = (planes, channels, d, dims, int(order), int(bool(relative)), mask, SOBOLEV_REDUCE[reduce], inv2h, invh,
            float(math.prod(hs)))
    nws = _lib.lib().fno_sobolev_loss_workspace_bytes(planes, d, dims, int(order))
    result = tuple(lead if reduce is None else lead[1:])
    if squeeze:
        result = tuple(n for n in result if n != 1)
    return scal, nws, planes, channels, result


class _SobolevLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, y, d, h, order, relative, fix, reduce, squeeze):
        _require_cuda(x, "x")
        scal, nws, planes, channels, result = _sobolev_plan(tuple(x.shape), d, h, order, relative, fix, reduce, squeeze)
        x_c = x.contiguous()
        y_c = _operand("sobolev_loss", "y", y, x, shape=x.shape)
        ws = _bytes(nws, x.device)
        out = torch.empty(planes + channels, dtype=torch.float32, device=x.device)
        value, reduced = out[:planes], out[planes:]
        _call("sobolev_loss_forward", x.device, "fno_sobolev_loss_forward", *scal, x_c, y_c, value,
              None if reduce is None else reduced, ws, nws, STREAM)
        ctx.save_for_backward(x_c, y_c, ws)
        ctx.meta = (scal, nws, x.shape, channels if reduce else planes)
        return (value if reduce is None else reduced).view(result)

    @staticmethod
    def backward(ctx, g):
        x_c, y_c, ws = ctx.saved_tensors
        scal, nws, shape, ngrad = ctx.meta
        grad = _operand("sobolev_loss backward", "grad", g.to(torch.float32), x_c, numel=ngrad)
        dx = torch.empty_like(x_c)
        _call("sobolev_loss_backward", dx.device, "fno_sobolev_loss_backward", *scal, x_c, y_c, grad, dx, ws, nws, STREAM)
        return dx.view(shape), None, None, None, None, None, None, None, None


def sobolev_loss(x, y, d, h, order=1, relative=True, fix=None, reduce=None, squeeze=False):
    """LpLoss (order 0, p = 2) / H1Loss (order 1) of neuralop/training/losses.py in one fused forward (two launches) and one
    backward launch.  x, y (*lead, n_1 .. n_d) float32 on the GPU, h the d step sizes, fix the d per-axis flags of a
    non-periodic axis (fix_x_bnd first; default all periodic).  relative: sqrt(num / den), else sqrt(prod(h) num).
    reduce None: the per-plane tensor `lead`; 'sum' / 'mean': reduced over the FIRST leading axis inside the engine, shape
    lead[1:]; squeeze: without the result's singleton axes (the reference's `.squeeze()`).  Differentiable w.r.t. x
    (non-contiguous inputs are copied); y is data.  A plane with x == y exactly gets a zero gradient (the reference's autograd
    gives NaN there)."""
    if y.requires_grad:
        raise _refuse("sobolev_loss", "y", "be data (the loss is differentiated with respect to `x` only)", "requires_grad=True")
    fix = (False,) * d if fix is None and isinstance(d, int) else fix
    return _SobolevLossFn.apply(x, y, d, tuple(float(v) for v in h), int(order), bool(relative), tuple(bool(f) for f in fix),
                                reduce, bool(squeeze))


# ----------------------------------------------------------------------------
# spectral Sobolev loss of the original FNO code base (HsLoss: libs/utilities3.py:339-405)
# ----------------------------------------------------------------------------
HS_REDUCE = {None: 0, "sum": 1, "mean": 2}        # csrc/k_hs_loss.h HS_REDUCE_*
HS_GRIDS = (32, 64, 128)                          # square planes the in-LDS transforms of csrc/k_hs_loss.h cover
HS_TERMS = 3                                      # |k|^0, |k|^2, |k|^4


def hs_loss_supported(x):
    """what k_hs_loss.h takes: float32 on the GPU, (B, N, N, *rest) with N = 32, 64 or 128, at least one sample and one
    channel (the trailing dimensions fold into one channel axis)"""
    return bool(x.is_cuda and x.dtype == torch.float32 and x.dim() >= 3 and x.shape[1] == x.shape[2] and x.shape[1] in HS_GRIDS
                and x.shape[0] >= 1 and math.prod(x.shape[3:]) >= 1)


@functools.lru_cache(maxsize=256)
def _hs_plan(shape, k, a, group, reduce):
    """The host's part of one configuration, worked out once: (the scalar arguments of both entry points, workspace bytes,
    batch).  The squared coefficients are float64 here."""
    e = "hs_loss"
    if len(shape) < 3 or shape[1] != shape[2] or shape[1] not in HS_GRIDS:
        raise _refuse(e, "x", f"be (B, N, N, ...) with a square plane of N = {', '.join(map(str, HS_GRIDS))} points a side "
                      "(the in-LDS transforms; there is no other path)", f"shape {tuple(shape)}")
    B, channels = shape[0], math.prod(shape[3:])
    if B < 1 or channels < 1:
        raise _refuse(e, "x", "have at least one sample and one channel", f"shape {tuple(shape)}")
    if not isinstance(k, int) or k < 0:
        raise _refuse(e, "k", "be a non-negative integer", repr(k))
    if reduce not in HS_REDUCE:
        raise _refuse(e, "reduce", "be None, 'sum' or 'mean'", repr(reduce))
    terms = min(k, HS_TERMS - 1) + 1
    if len(a) < terms - 1:
        raise _refuse(e, "a", f"have a coefficient for each of the orders 1 .. {terms - 1}", f"a={list(a)}, k={k}")
    w2 = (C.c_double * HS_TERMS)(1.0, *[float(v) ** 2 for v in a[:terms - 1]])
    scal = (B, shape[1], shape[2], channels, terms, w2, int(group), float(k + 1), HS_REDUCE[reduce])
    return scal, _lib.lib().fno_hs_loss_workspace_bytes(B, channels), B


class _HsLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, y, k, a, group, reduce):
        scal, nws, B = _hs_plan(tuple(x.shape), k, a, group, reduce)
        _require_cuda(x, "x")
        x_c = x.contiguous()
        y_c = _operand("hs_loss", "y", y, x, shape=x.shape)
        ws = _bytes(nws, x.device)
        out = torch.empty(B + 1, dtype=torch.float32, device=x.device)
        value, reduced = out[:B], out[B:]
        _call("hs_loss_forward", x.device, "fno_hs_loss_forward", *scal, x_c, y_c, value, None if reduce is None else reduced,
              ws, nws, STREAM)
        ctx.save_for_backward(x_c, y_c, ws)
        ctx.meta = (scal, nws, x.shape, B if reduce is None else 1)
        return value if reduce is None else reduced.view(())

    @staticmethod
    def backward(ctx, g):
        x_c, y_c, ws = ctx.saved_tensors
        scal, nws, shape, ngrad = ctx.meta
        grad = _operand("hs_loss backward", "grad", g.to(torch.float32), x_c, numel=ngrad)
        dx = torch.empty_like(x_c)
        _call("hs_loss_backward", dx.device, "fno_hs_loss_backward", *scal, x_c, y_c, grad, dx, ws, nws, STREAM)
        return dx.view(shape), None, None, None, None, None


def hs_loss(x, y, k=1, a=None, group=False, reduce="mean"):
    """HsLoss of libs/utilities3.py:339-405 in one fused forward (two launches) and one backward launch.  x, y (B, N, N, *rest)
    float32 on the GPU, channels last, N = 32, 64 or 128; the loss compares them in Fourier space with the weights
    1 + a[0]^2 |k|^2 + a[1]^2 |k|^4 (orders up to min(k, 2); a defaults to [1] * k); group: the mean of the per-order relative
    norms over k + 1 instead of one weighted norm.  reduce 'mean' / 'sum': a 0-d tensor, reduced over the batch inside the engine;
    None: the (B,) values.  Differentiable w.r.t. x (non-contiguous inputs are copied); y is data.  A sample with x == y exactly
    gets a zero gradient (the reference's autograd gives NaN there).  Any other grid raises: there is no torch fallback."""
    if y.requires_grad:
        raise _refuse("hs_loss", "y", "be data (the loss is differentiated with respect to `x` only)", "requires_grad=True")
    if not isinstance(k, int) or isinstance(k, bool) or k < 0:
        raise _refuse("hs_loss", "k", "be a non-negative integer", repr(k))
    a = (1.0,) * k if a is None else a
    return _HsLossFn.apply(x, y, k, tuple(float(v) for v in a), bool(group), reduce)
