"""Single fused layers around the Fourier stacks: RNO gates, pointwise convolutions, lifting, the spectral + pointwise layer,
the projection head, the channel MLP, domain padding.
"""
import ctypes as C

import torch

from .. import _lib
from ._core import _bytes, _call, _operand, _plan_available, plane_size, _ptr_array, _refuse, _require_cuda, STREAM
from .spectral import _check_corner_weights, _direct_views, _fresh_grads, _notify_direct, _real_views, spec_plan, _spec_plans


# ----------------------------------------------------------------------------
# RNO cell gates (neuralop/models/rno.py:254-260)
# ----------------------------------------------------------------------------
def gates_supported(*tensors):
    t0 = tensors[0]
    return all(t.is_cuda and t.dtype == torch.float32 and t.shape == t0.shape for t in tensors) and t0.numel() % 4 == 0


def _gate_operands(e, h, fields, scalars):
    """the operands of an RNO gate: `fields` (name -> tensor) of the state's shape, `scalars` (name -> tensor) one float each"""
    _require_cuda(h, "h")
    return ([_operand(e, n, t, h, shape=h.shape) for n, t in fields] + [h.contiguous()],
            [_operand(e, n, t, h, numel=1) for n, t in scalars])


class _RnoResetGateFn(torch.autograd.Function):
    """rh = sigmoid(a3 + a4 + b2) * h."""

    @staticmethod
    def forward(ctx, a3, a4, b2, h):
        (a3, a4, h), (b2,) = _gate_operands("rno_reset_gate", h, (("a3", a3), ("a4", a4)), (("b2", b2),))
        r, rh = torch.empty_like(h), torch.empty_like(h)
        _call("rno_reset_gate_forward", h.device, "fno_rno_reset_gate_forward", h.numel(), a3, a4, b2, h, r, rh, STREAM)
        ctx.save_for_backward(r, h)
        return rh

    @staticmethod
    def backward(ctx, d_rh):
        r, h = ctx.saved_tensors
        d_rh = _operand("rno_reset_gate backward", "d_rh", d_rh, h, shape=h.shape)
        ds, dh = torch.empty_like(h), torch.empty_like(h)
        part = torch.empty(_lib.lib().fno_rno_gate_partials(), dtype=torch.float64, device=h.device)
        _call("rno_reset_gate_backward", h.device, "fno_rno_reset_gate_backward", h.numel(), d_rh, r, h, ds, dh, part, STREAM)
        return ds, ds, part.sum().float().reshape(()), dh


class _RnoOutputGateFn(torch.autograd.Function):
    """h_new = (1 - sigmoid(a1 + a2 + b1)) * h + sigmoid(a7 + a8 + b4) * selu(a5 + a6 + b3)."""

    @staticmethod
    def forward(ctx, a1, a2, b1, a7, a8, b4, a5, a6, b3, h):
        (a1, a2, a7, a8, a5, a6, h), (b1, b4, b3) = _gate_operands(
            "rno_output_gate", h, (("a1", a1), ("a2", a2), ("a7", a7), ("a8", a8), ("a5", a5), ("a6", a6)),
            (("b1", b1), ("b4", b4), ("b3", b3)))
        z, z2, s3, hn = (torch.empty_like(h) for _ in range(4))
        _call("rno_output_gate_forward", h.device, "fno_rno_output_gate_forward", h.numel(), a1, a2, b1, a7, a8, b4, a5, a6, b3, h,
              z, z2, s3, hn, STREAM)
        ctx.save_for_backward(z, z2, s3, h)
        return hn

    @staticmethod
    def backward(ctx, g):
        z, z2, s3, h = ctx.saved_tensors
        g = _operand("rno_output_gate backward", "g", g, h, shape=h.shape)
        d1, d7, d3, dh = (torch.empty_like(h) for _ in range(4))
        P = _lib.lib().fno_rno_gate_partials()
        part = torch.empty(3, P, dtype=torch.float64, device=h.device)
        _call("rno_output_gate_backward", h.device, "fno_rno_output_gate_backward", h.numel(), g, z, z2, s3, h, d1, d7, d3, dh,
              part, STREAM)
        db = part.sum(dim=1).float()
        return d1, d1, db[0].reshape(()), d7, d7, db[1].reshape(()), d3, d3, db[2].reshape(()), dh


def rno_reset_gate(a3, a4, b2, h):
    return _RnoResetGateFn.apply(a3, a4, b2, h)


def rno_output_gate(a1, a2, b1, a7, a8, b4, a5, a6, b3, h):
    return _RnoOutputGateFn.apply(a1, a2, b1, a7, a8, b4, a5, a6, b3, h)


# ----------------------------------------------------------------------------
# pointwise channel mix + bias + residual add (the Conv1d(k=1) beside a spectral convolution)
# ----------------------------------------------------------------------------
def pointwise_supported(x):
    if not (x.is_cuda and x.dtype == torch.float32 and x.dim() >= 3):
        return False
    return x.shape[1] in (32, 64) and plane_size(x.shape) % 128 == 0


class _PointwiseAddFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, bias, addend):
        e = "pointwise_conv_add"
        _require_cuda(x, "x")
        x = x.contiguous()
        B, Cc = x.shape[0], x.shape[1]
        pw = x.numel() // (B * Cc)
        w2 = _operand(e, "w", w, x, numel=Cc * Cc).reshape(Cc, Cc)
        add_c = _operand(e, "addend", addend, x, shape=x.shape, optional=True)
        b_c = _operand(e, "bias", bias, x, numel=Cc, optional=True)
        y = torch.empty_like(x)
        _call("pointwise_forward", x.device, "fno_pointwise_forward", B, Cc, pw, x, w2, b_c, add_c, 0, y, STREAM)
        ctx.save_for_backward(x, w2)
        ctx.meta = (B, Cc, pw, w.shape, bias is not None, addend is not None)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w2 = ctx.saved_tensors
        B, Cc, pw, wshape, has_b, has_add = ctx.meta
        dy = _operand("pointwise_conv_add backward", "dy", dy, x, numel=x.numel())
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        dw = torch.empty_like(w2)
        db = torch.empty(Cc, dtype=torch.float32, device=x.device) if has_b else None
        nws = _lib.lib().fno_pointwise_workspace_bytes(Cc)
        ws = _bytes(nws, x.device)
        _call("pointwise_backward", x.device, "fno_pointwise_backward", B, Cc, pw, x, w2, dy, None, 0, dx, dw, db, ws, nws, STREAM)
        return dx, dw.view(wshape), db, (dy if has_add else None)


def pointwise_conv_add(x, w, bias=None, addend=None):
    """y = conv1x1(x; w) + bias + addend  (x, addend (B, C, ...), w (C, C[, 1..]), C in {32, 64}) in one engine
    kernel each way; the gradient of `addend` is the incoming gradient itself."""
    return _PointwiseAddFn.apply(x, w, bias, addend)


class _PointwisePerSampleFn(torch.autograd.Function):
    """y[b] = conv1x1(x[b]; w) + bias[b]: the channel mix with a PER-SAMPLE bias row (B, C) - the Re-conditioning affine
    `B x + A re + bias` of the PINO observers (pinobserver.py:41-59), whose per-sample code `A re` would otherwise cost a
    broadcast-add pass over the whole tensor (and a reduction pass in backward).  One fno_pointwise_* call per sample."""

    @staticmethod
    def forward(ctx, x, w, bias):
        e = "pointwise_conv_per_sample_bias"
        _require_cuda(x, "x")
        x = x.contiguous()
        B, Cc = x.shape[0], x.shape[1]
        pw = x.numel() // (B * Cc)
        w2 = _operand(e, "w", w, x, numel=Cc * Cc).reshape(Cc, Cc)
        bc = _operand(e, "bias", bias, x, shape=(B, Cc))
        y = torch.empty_like(x)
        for b in range(B):
            _call("pointwise_forward", x.device, "fno_pointwise_forward", 1, Cc, pw, x[b], w2, bc[b], None, 0, y[b], STREAM)
        ctx.save_for_backward(x, w2)
        ctx.meta = (B, Cc, pw, w.shape)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w2 = ctx.saved_tensors
        B, Cc, pw, wshape = ctx.meta
        dy = _operand("pointwise_conv_per_sample_bias backward", "dy", dy, x, numel=x.numel())
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        dws = torch.empty((B, Cc, Cc), dtype=torch.float32, device=x.device)
        dbs = torch.empty((B, Cc), dtype=torch.float32, device=x.device)
        nws = _lib.lib().fno_pointwise_workspace_bytes(Cc)
        ws = _bytes(nws, x.device)
        for b in range(B):
            _call("pointwise_backward", x.device, "fno_pointwise_backward", 1, Cc, pw, x[b], w2, dy[b], None, 0,
                  dx[b] if dx is not None else None, dws[b], dbs[b], ws, nws, STREAM)
        return dx, dws.sum(0).view(wshape), dbs


def pointwise_conv_per_sample_bias(x, w, bias):
    """y[b] = conv1x1(x[b]; w) + bias[b] with bias (B, C); x (B, C, ...), C in {32, 64}."""
    return _PointwisePerSampleFn.apply(x, w, bias)


# ----------------------------------------------------------------------------
# lifting layer  y = W x + b,  (B, Cin <= 4, ...) -> (B, C, ...); bias one row (C) or one row per sample (B, C)
# ----------------------------------------------------------------------------
def lifting_supported(x, c_out):
    if not (x.is_cuda and x.dtype == torch.float32 and x.dim() >= 3 and 1 <= x.shape[1] <= 4 and c_out in (32, 64)):
        return False
    return plane_size(x.shape) % 128 == 0


def _lifting_operands(e, x, w, bias, per_sample):
    """-> x contiguous, (B, cin, cout, pw), w (cout, cin), bias (None allowed unless per_sample)"""
    _require_cuda(x, "x")
    x = x.contiguous()
    B, cin, cout = x.shape[0], x.shape[1], w.shape[0]
    wc = _operand(e, "w", w, x, numel=cout * cin).reshape(cout, cin)
    bc = _operand(e, "bias", bias, x, shape=(B, cout)) if per_sample else _operand(e, "bias", bias, x, numel=cout, optional=True)
    return x, (B, cin, cout, x.numel() // (B * cin)), wc, bc


def _lifting_dx(ctx, x, wc, dy, B, cin, cout, pw):
    """dL/dx of a lifting when the input asks for it (fno_lifting_backward_dx: channels summed in ascending order), else None"""
    if not ctx.needs_input_grad[0]:
        return None
    dx = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    _call("lifting_backward_dx", x.device, "fno_lifting_backward_dx", B, cin, cout, pw, dy, wc, dx, STREAM)
    return dx


class _LiftingPerSampleFn(torch.autograd.Function):
    """lifting with a per-sample bias row (B, C): one fno_lifting_* call per sample (see _PointwisePerSampleFn)."""

    @staticmethod
    def forward(ctx, x, w, bias):
        x, (B, cin, cout, pw), wc, bc = _lifting_operands("lifting_per_sample_bias", x, w, bias, True)
        y = torch.empty((B, cout) + tuple(x.shape[2:]), dtype=torch.float32, device=x.device)
        for b in range(B):
            _call("lifting_forward", x.device, "fno_lifting_forward", 1, cin, cout, pw, x[b], wc, bc[b], y[b], STREAM)
        ctx.save_for_backward(x, wc)
        ctx.meta = (B, cin, cout, pw, w.shape)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, wc = ctx.saved_tensors
        B, cin, cout, pw, wshape = ctx.meta
        dy = _operand("lifting_per_sample_bias backward", "dy", dy, x, numel=B * cout * pw)
        dx = _lifting_dx(ctx, x, wc, dy, B, cin, cout, pw)
        if not (ctx.needs_input_grad[1] or ctx.needs_input_grad[2]):
            return dx, None, None
        dws = torch.empty((B, cout, cin), dtype=torch.float32, device=x.device)
        dbs = torch.empty((B, cout), dtype=torch.float32, device=x.device)
        nws = _lib.lib().fno_lifting_workspace_bytes(cout)
        ws = _bytes(nws, x.device)
        for b in range(B):
            _call("lifting_backward", x.device, "fno_lifting_backward", 1, cin, cout, pw, x[b], dy[b], dws[b], dbs[b], ws, nws,
                  STREAM)
        return dx, dws.sum(0).view(wshape), dbs


def lifting_per_sample_bias(x, w, bias):
    """y[b] = conv1x1(x[b]; w) + bias[b]: x (B, Cin <= 4, ...), w (C, Cin), bias (B, C).  dL/dx is produced when x asks for it."""
    return _LiftingPerSampleFn.apply(x, w, bias)


class _LiftingFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, bias):
        x, (B, cin, cout, pw), wc, bc = _lifting_operands("lifting", x, w, bias, False)
        y = torch.empty((B, cout) + tuple(x.shape[2:]), dtype=torch.float32, device=x.device)
        _call("lifting_forward", x.device, "fno_lifting_forward", B, cin, cout, pw, x, wc, bc, y, STREAM)
        ctx.save_for_backward(x, wc)
        ctx.meta = (B, cin, cout, pw, w.shape, bias is not None)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, wc = ctx.saved_tensors
        B, cin, cout, pw, wshape, has_b = ctx.meta
        dy = _operand("lifting backward", "dy", dy, x, numel=B * cout * pw)
        dx = _lifting_dx(ctx, x, wc, dy, B, cin, cout, pw)
        if not (ctx.needs_input_grad[1] or ctx.needs_input_grad[2]):      # frozen parameters: only the input gradient is formed
            return dx, None, None
        dw = torch.empty(cout, cin, dtype=torch.float32, device=x.device)
        db = torch.empty(cout, dtype=torch.float32, device=x.device) if has_b else None
        nws = _lib.lib().fno_lifting_workspace_bytes(cout)
        ws = _bytes(nws, x.device)
        _call("lifting_backward", x.device, "fno_lifting_backward", B, cin, cout, pw, x, dy, dw, db, ws, nws, STREAM)
        return dx, dw.view(wshape), db


def lifting(x, w, bias=None):
    """conv1x1 from <= 4 input channels: x (B, Cin, ...), w (C, Cin[, 1..]), bias (C).  dL/dx = W^T dL/dy is produced when x
    asks for it (the optimal-observer policy differentiates an observer down to its input field)."""
    return _LiftingFn.apply(x, w, bias)


class _ZeroLastPadsFn(torch.autograd.Function):
    """Zero the first p0 and last p1 entries of the last dimension IN PLACE, forward and backward: makes a tensor that was
    computed on a zero-padded INPUT equal to the zero-padded tensor the reference builds with F.pad after the fact
    (pinobserver.py:208-213), without the pad copy (forward) or the slice copy (backward)."""

    @staticmethod
    def forward(ctx, y, p0, p1):
        ctx.pads = (p0, p1)
        ctx.mark_dirty(y)
        if p0 > 0:
            y[..., :p0].zero_()
        if p1 > 0:
            y[..., y.shape[-1] - p1:].zero_()
        return y

    @staticmethod
    def backward(ctx, g):
        p0, p1 = ctx.pads
        g = g.contiguous()          # the block stack's input gradient: a fresh tensor with no other consumer
        if p0 > 0:
            g[..., :p0].zero_()
        if p1 > 0:
            g[..., g.shape[-1] - p1:].zero_()
        return g, None, None


def zero_last_pads_(y, p0, p1):
    return _ZeroLastPadsFn.apply(y, int(p0), int(p1))


# ----------------------------------------------------------------------------
# one layer of the observer stacks:  y = SpectralConv(a) + Conv1d_{k=1}(a) + bias,  a = gelu(u) or u
# ----------------------------------------------------------------------------
def spectral_layer_supported(u, n_spec_weights, modes, norm, weight_last_extent, input_gelu):
    """True when spectral_pointwise_layer can run this shape (result cached per shape)."""
    if not pointwise_supported(u) or n_spec_weights != 2 ** (u.dim() - 3):
        return False
    key = ("layer", u.dim() - 2, u.shape[1], tuple(u.shape[2:]), tuple(modes), weight_last_extent, norm, u.device.index, bool(input_gelu))
    return _plan_available(_spec_plans, key, spec_plan, u.dim() - 2, u.shape[1], u.shape[1], tuple(u.shape[2:]), modes,
                           weight_last_extent, norm, u.device, input_gelu)


class _SpectralLayerFn(torch.autograd.Function):
    """forward: sp = fno_spec_forward(u) [gelu on load], y = fno_pointwise_forward(u, addend = sp) [gelu on load].
    backward: (d_a from the spectral branch, dW_spec) = fno_spec_backward(dy); fno_pointwise_backward adds it to W^T dy,
    applies gelu'(u) and writes du: no separate activation, activation-derivative or gradient-accumulation pass."""

    @staticmethod
    def forward(ctx, u, w, bias, modes, norm, wle, input_gelu, direct, *spec_ws):
        e = "spectral_pointwise_layer"
        _require_cuda(u, "u")
        u = u.contiguous()
        B, Cc = u.shape[0], u.shape[1]
        dims = tuple(u.shape[2:])
        pw = u.numel() // (B * Cc)
        if len(spec_ws) != 2 ** (len(dims) - 1) or len(modes) != len(dims):
            raise RuntimeError(f"fnoengine {e}: {len(spec_ws)} corner weights / {len(modes)} mode counts for {len(dims)}-d data")
        ws_list, planes = _check_corner_weights(e, spec_ws, u, Cc, Cc, modes, last=wle)
        ctx.planes = planes
        w2 = _operand(e, "w", w, u, numel=Cc * Cc).reshape(Cc, Cc)
        b_c = _operand(e, "bias", bias, u, numel=Cc, optional=True)
        L = _lib.lib()
        plan = spec_plan(len(dims), Cc, Cc, dims, modes, wle, norm, u.device, input_gelu, weight_planes=planes)
        sp = torch.empty_like(u)
        xhat = _bytes(L.fno_spec_xhat_bytes(plan, B), u.device)
        nws = L.fno_spec_workspace_bytes(plan, B)
        ws = _bytes(nws, u.device)
        y = torch.empty_like(u)
        _call("spec_forward", u.device, "fno_spec_forward", plan, B, u, _ptr_array(ws_list, 4), None, sp, xhat, ws, nws, STREAM)
        _call("pointwise_forward", u.device, "fno_pointwise_forward", B, Cc, pw, u, w2, b_c, sp, 1 if input_gelu else 0, y, STREAM)
        ctx.plan, ctx.meta, ctx.direct = plan, (B, Cc, pw, w.shape, bias is not None, bool(input_gelu)), direct
        ctx.save_for_backward(u, w2, xhat, *ws_list)
        return y

    @staticmethod
    def backward(ctx, dy):
        u, w2, xhat, *ws_list = ctx.saved_tensors
        B, Cc, pw, wshape, has_b, input_gelu = ctx.meta
        L = _lib.lib()
        dy = _operand("spectral_pointwise_layer backward", "dy", dy, u, numel=u.numel())
        need_du = ctx.needs_input_grad[0]
        need_dws = any(ctx.needs_input_grad[8:])
        direct = ctx.direct if need_dws else None
        dws = (direct if direct is not None else _fresh_grads(ws_list, ctx.planes)) if need_dws else None
        da = torch.empty_like(u) if need_du else None           # gradient reaching gelu(u) through the spectral branch
        du = torch.empty_like(u) if need_du else None
        dw = torch.empty_like(w2)
        db = torch.empty(Cc, dtype=torch.float32, device=u.device) if has_b else None
        nws = L.fno_spec_workspace_bytes(ctx.plan, B)
        ws = _bytes(nws, u.device)
        nws2 = L.fno_pointwise_workspace_bytes(Cc)
        ws2 = _bytes(nws2, u.device)
        _call("spec_backward", u.device, "fno_spec_backward", ctx.plan, B, dy, xhat, None, da, _ptr_array(dws, 4), None, ws, nws,
              STREAM)
        _call("pointwise_backward", u.device, "fno_pointwise_backward", B, Cc, pw, u, w2, dy, da, 1 if input_gelu else 0, du, dw,
              db, ws2, nws2, STREAM)
        gw = (None,) * len(ws_list) if (direct is not None or not need_dws) else tuple(dws)
        if direct is not None:
            _notify_direct(direct)
        return (du, dw.view(wshape), db, None, None, None, None, None) + gw


def spectral_pointwise_layer(u, spec_weights, modes, norm, w, bias, input_gelu=False, weight_last_extent=None,
                             direct_grads=False):
    """y = SpectralConv(a) + Conv1d_{k=1}(a; w) + bias with a = gelu(u) if input_gelu else u: one layer of the observer
    stacks (libs/models/pino_models/pinobserver.py:221-226) with the PREVIOUS layer's activation applied while u is
    loaded, so a stack is chained on pre-activation tensors.  Check spectral_layer_supported() first."""
    sw = _real_views(spec_weights)
    wle = int(weight_last_extent) if weight_last_extent is not None else int(sw[0].shape[-2])
    direct = _direct_views(direct_grads, spec_weights, last_dim=u.shape[-1])
    return _SpectralLayerFn.apply(u, w, bias, tuple(int(m) for m in modes), norm, wle, bool(input_gelu), direct, *sw)


# ----------------------------------------------------------------------------
# projection head  y = W2 gelu(W1 x + b1) + b2  on (B, C, ...) tensors
# ----------------------------------------------------------------------------
PROJ_MAXCO = 4        # k_projection.h
_ACT_CODES = {"gelu": _lib.ABI.consts["FNO_ACT_GELU"], "relu": _lib.ABI.consts["FNO_ACT_RELU"]}


def projection_supported(x, hidden, cout, act="gelu"):
    return (pointwise_supported(x) and hidden in ((128, 256) if act == "gelu" else (256,))
            and (cout == 1 or (act == "gelu" and 1 <= cout <= PROJ_MAXCO))
            and act in _ACT_CODES)


class _ProjectionHeadFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, act=0):
        e = "projection_head"
        _require_cuda(x, "x")
        x = x.contiguous()
        B, Cc = x.shape[0], x.shape[1]
        pw = x.numel() // (B * Cc)
        hid, co = w1.shape[0], w2.shape[0]
        w1c = _operand(e, "w1", w1, x, numel=hid * Cc).reshape(hid, Cc)
        b1c = _operand(e, "b1", b1, x, numel=hid)
        w2c = _operand(e, "w2", w2, x, numel=co * hid).reshape(co, hid)
        b2c = _operand(e, "b2", b2, x, numel=co)
        y = torch.empty((B, co) + tuple(x.shape[2:]), dtype=torch.float32, device=x.device)
        _call("projection_forward", x.device, "fno_projection_forward_act", B, Cc, hid, co, pw, x, w1c, b1c, w2c, b2c, act, y,
              STREAM)
        ctx.save_for_backward(x, w1c, b1c, w2c)
        ctx.meta = (B, Cc, hid, pw, w1.shape, w2.shape, act, co)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w1c, b1c, w2c = ctx.saved_tensors
        B, Cc, hid, pw, w1shape, w2shape, act, co = ctx.meta
        dy = _operand("projection_head backward", "dy", dy, x, numel=B * co * pw)
        dx = torch.empty_like(x)
        dw1, db1, dw2 = torch.empty_like(w1c), torch.empty_like(b1c), torch.empty_like(w2c)
        db2 = torch.empty(co, dtype=torch.float32, device=x.device)
        nws = _lib.lib().fno_projection_workspace_bytes(Cc, hid)
        ws = _bytes(nws, x.device)
        _call("projection_backward", x.device, "fno_projection_backward_act", B, Cc, hid, co, pw, x, w1c, b1c, w2c, dy, act, dx,
              dw1, db1, dw2, db2, ws, nws, STREAM)
        return dx, dw1.view(w1shape), db1, dw2.view(w2shape), db2, None


def projection_head(x, w1, b1, w2, b2, act="gelu"):
    """(B, C, ...) -> (B, Cout, ...): fc2(act(fc1(x))) with fc1.weight (hidden, C), fc2.weight (Cout, hidden); act 'gelu'
    (FNO projection, PINO observer tails; Cout <= 4: PlanePredHead's out_dim * plane_num, pinobserver.py:257-273) or 'relu'
    (RNO2d's regressor head, rno.py:171-175; hidden 256, Cout 1)."""
    return _ProjectionHeadFn.apply(x, w1, b1, w2, b2, _ACT_CODES[act])


# ----------------------------------------------------------------------------
# channel MLP of an FNO block built with use_mlp=True:  y = [gelu]( gelu(W2 gelu(W1 u + b1) + b2) + gate * x )
# ----------------------------------------------------------------------------
CHANNEL_MLP_WIDTHS = ((64, 32), (64, 64), (32, 32))        # (channels, hidden) pairs k_channel_mlp.h is built for


def channel_mlp_supported(x, hidden):
    return (x.is_cuda and x.dtype == torch.float32 and x.dim() >= 3 and (x.shape[1], int(hidden)) in CHANNEL_MLP_WIDTHS
            and plane_size(x.shape) % 128 == 0)


class _ChannelMlpFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, u, x, w1, b1, w2, b2, gate, gelu_out):
        e = "channel_mlp"
        _require_cuda(u, "u")
        u = u.contiguous()
        B, Cc = u.shape[0], u.shape[1]
        pw = u.numel() // (B * Cc)
        hid = w1.shape[0]
        xc = _operand(e, "x", x, u, shape=u.shape)
        w1c = _operand(e, "w1", w1, u, numel=hid * Cc).reshape(hid, Cc)
        b1c = _operand(e, "b1", b1, u, numel=hid)
        w2c = _operand(e, "w2", w2, u, numel=Cc * hid).reshape(Cc, hid)
        b2c = _operand(e, "b2", b2, u, numel=Cc)
        gc = _operand(e, "gate", gate, u, numel=Cc, optional=True)
        y = torch.empty_like(u)
        _call("channel_mlp_forward", u.device, "fno_channel_mlp_forward", B, Cc, hid, pw, u, xc, w1c, b1c, w2c, b2c, gc,
              int(bool(gelu_out)), y, STREAM)
        ctx.save_for_backward(u, xc, w1c, b1c, w2c, b2c, *(() if gc is None else (gc,)))
        ctx.meta = (B, Cc, hid, pw, w1.shape, w2.shape, None if gate is None else gate.shape, int(bool(gelu_out)))
        return y

    @staticmethod
    def backward(ctx, dy):
        u, xc, w1c, b1c, w2c, b2c, *rest = ctx.saved_tensors
        gc = rest[0] if rest else None
        B, Cc, hid, pw, w1shape, w2shape, gshape, gelu_out = ctx.meta
        dy = _operand("channel_mlp backward", "dy", dy, u, numel=u.numel())
        du = torch.empty_like(u)
        dx = torch.empty_like(xc) if ctx.needs_input_grad[1] else None
        dw1, db1, dw2, db2 = torch.empty_like(w1c), torch.empty_like(b1c), torch.empty_like(w2c), torch.empty_like(b2c)
        dg = None if gc is None else torch.empty_like(gc)
        nws = _lib.lib().fno_channel_mlp_workspace_bytes(Cc, hid, B, pw)
        ws = _bytes(nws, u.device)
        _call("channel_mlp_backward", u.device, "fno_channel_mlp_backward", B, Cc, hid, pw, u, xc, w1c, b1c, w2c, b2c, gc,
              gelu_out, dy, du, dx, dw1, db1, dw2, db2, dg, ws, nws, STREAM)
        return (du, dx, dw1.view(w1shape), db1, dw2.view(w2shape), db2, None if dg is None else dg.view(gshape), None)


def channel_mlp(u, x, w1, b1, w2, b2, gate=None, gelu_out=False):
    """The MLP tail of an FNO block (fno_block.py:137-169 with use_mlp=True): (B, C, ...) -> (B, C, ...),
    gelu(fcs.1(gelu(fcs.0(u)))) + gate * x, GELU on the sum when `gelu_out`.  u: the Fourier part's output, x: the block's
    input, w1 (H, C[, 1..]), w2 (C, H[, 1..]), gate (C) / (1, C, 1..) or None (identity skip); (C, H) in CHANNEL_MLP_WIDTHS.
    One kernel per direction; the backward recomputes the intermediates from u and x and skips dx when x needs no gradient."""
    return _ChannelMlpFn.apply(u, x, w1, b1, w2, b2, gate, gelu_out)


# ----------------------------------------------------------------------------
# domain padding: zero-pad the grid of a (B, C, d1[, d2[, d3]]) tensor, or crop the interior back out
# ----------------------------------------------------------------------------
def _domain_amounts(e, ndim, before, after):
    """`before` / `after` as ndim-tuples of non-negative ints (an int stands for every axis)"""
    out = []
    for name, v in (("before", before), ("after", after)):
        v = (int(v),) * ndim if isinstance(v, int) else tuple(int(p) for p in v)
        if len(v) != ndim or min(v) < 0:
            raise _refuse(e, name, f"be {ndim} non-negative amounts, one per grid axis", v)
        out.append(v)
    return out


def _domain_move(e, fname, src, dims, before, after, out_dims):
    """one fno_domain_pad / fno_domain_crop call on a checked, contiguous `src` (B, C, ...): -> (B, C) + out_dims"""
    ndim = len(dims)
    ints = C.c_int * ndim
    dst = torch.empty(tuple(src.shape[:2]) + tuple(out_dims), dtype=torch.float32, device=src.device)
    _call(e, src.device, fname, ndim, src.shape[0] * src.shape[1], ints(*dims), ints(*before), ints(*after), src, dst, STREAM)
    return dst


def _domain_operand(e, name, t):
    _require_cuda(t, name)
    if not 3 <= t.dim() <= 5:
        raise _refuse(e, name, "be (B, C, d1[, d2[, d3]])", tuple(t.shape))
    return t.contiguous()


class _DomainPadFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, before, after):
        e = "domain_pad"
        x = _domain_operand(e, "x", x)
        dims = tuple(x.shape[2:])
        before, after = _domain_amounts(e, len(dims), before, after)
        ctx.meta = (dims, before, after)
        return _domain_move(e, "fno_domain_pad", x, dims, before, after, [d + b + a for d, b, a in zip(dims, before, after)])

    @staticmethod
    def backward(ctx, dy):
        e = "domain_pad backward"
        dims, before, after = ctx.meta
        dy = _domain_operand(e, "dy", dy)
        if tuple(dy.shape[2:]) != tuple(d + b + a for d, b, a in zip(dims, before, after)):
            raise _refuse(e, "dy", "have the padded grid", tuple(dy.shape))
        return _domain_move(e, "fno_domain_crop", dy, dims, before, after, dims), None, None


class _DomainCropFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y, before, after):
        e = "domain_crop"
        y = _domain_operand(e, "y", y)
        before, after = _domain_amounts(e, y.dim() - 2, before, after)
        dims = tuple(p - b - a for p, b, a in zip(y.shape[2:], before, after))
        if min(dims) < 1:
            raise _refuse(e, "y", f"be larger than its pads {before} + {after} on every axis", tuple(y.shape))
        ctx.meta = (dims, before, after)
        return _domain_move(e, "fno_domain_crop", y, dims, before, after, dims)

    @staticmethod
    def backward(ctx, dx):
        e = "domain_crop backward"
        dims, before, after = ctx.meta
        dx = _domain_operand(e, "dx", dx)
        if tuple(dx.shape[2:]) != dims:
            raise _refuse(e, "dx", "have the cropped grid", tuple(dx.shape))
        return _domain_move(e, "fno_domain_pad", dx, dims, before, after, [d + b + a for d, b, a in zip(dims, before, after)]), None, None


def domain_pad(x, before, after):
    """Zero-pad the grid of x (B, C, d1[, d2[, d3]]): `before[d]` zeros in front of axis d and `after[d]` behind it (ints or one
    int for every axis).  One kernel (k_domain_pad) writes the whole result - interior copied bit for bit, margin +0.0; the
    backward is the crop of the gradient (k_domain_crop)."""
    return _DomainPadFn.apply(x, before, after)


def domain_crop(y, before, after):
    """The interior of a padded y (B, C, p1[, p2[, p3]]): drops `before[d]` leading and `after[d]` trailing entries of axis d.
    One kernel (k_domain_crop); the backward is the zero-pad of the gradient (k_domain_pad)."""
    return _DomainCropFn.apply(y, before, after)
