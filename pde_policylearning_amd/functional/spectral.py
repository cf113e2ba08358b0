"""The standalone spectral convolution, and what the plan-based Functions share: plan cache, corner weights, direct gradient
writes.  Home of _spec_plans, DIRECT_WRITE_HOOKS, _SINGLE_USE and LAST_FORWARD_SINGLE_USE (mutated in place, never rebound).
"""
import ctypes as C
import typing
import weakref

import torch

from .. import _lib
from ._core import _bytes, _call, _operand, _ptr, _ptr_array, _require_cuda, STREAM

_spec_plans = {}


class _Cfg(typing.NamedTuple):
    """the non-tensor argument of the three plan-based Functions"""
    n_layers: int
    modes: tuple
    norm: typing.Optional[str]
    gelu_mask: int = 0
    direct: typing.Any = None       # gradient storage the backward writes in place (_direct_views / fno_model), or None
    overlap: typing.Any = None      # fno_model: the trainer's exchange-overlap hook
    tail: typing.Any = None         # fno_block_tail: (relu_out, drop_p, seed tensor or None)


def _fill_params(ncorner, skip_ws, spec_ws, spec_bias=None, ends=None, struct=_lib.FnoModelParams):
    """FnoModelParams (`struct=_lib.FnoModelGrads`: the gradients, same fields) over checked tensors: per layer / fan-out member
    one skip weight and `ncorner` corner weights, the bias rows, and for the whole model `ends` = (lift_w, lift_b, proj_w1,
    proj_b1, proj_w2, proj_b2)."""
    s = struct()
    for l, t in enumerate(skip_ws):
        s.skip_w[l] = t.data_ptr()
        for c in range(ncorner):
            s.spec_w[l][c] = spec_ws[l * ncorner + c].data_ptr()
    s.spec_bias = _ptr(spec_bias)
    if ends is not None:
        s.lift_w, s.lift_b, s.proj_w1, s.proj_b1, s.proj_w2, s.proj_b2 = [t.data_ptr() for t in ends]
    return s


def _saved_params(sv, head, n_layers, ncorner, has_bias=False):
    """(skip weights, corner weights, bias rows or None) back out of saved_tensors, where they follow `head` other tensors"""
    a, b = head + n_layers, head + n_layers + n_layers * ncorner
    return list(sv[head:a]), list(sv[a:b]), sv[b] if has_bias else None


# ----------------------------------------------------------------------------
# standalone spectral convolution
# ----------------------------------------------------------------------------
def spec_plan(ndim, cin, cout, dims, modes, weight_last_extent, norm, device, input_gelu=False, weight_planes=False):
    key = (ndim, cin, cout, tuple(dims), tuple(modes), weight_last_extent, norm, device.index, bool(input_gelu),
           bool(weight_planes))
    plan = _spec_plans.get(key)
    if plan is None:
        d = _lib.FnoSpecDesc()
        d.ndim, d.Cin, d.Cout = ndim, cin, cout
        for i in range(ndim):
            d.dims[i], d.modes[i] = int(dims[i]), int(modes[i])
        d.weight_last_extent = int(weight_last_extent)
        d.norm = _lib.NORM_CODES[norm]
        d.input_gelu = 1 if input_gelu else 0
        d.weight_planes = 1 if weight_planes else 0
        plan = C.c_void_p()
        _call("spec_plan_create", device, "fno_spec_plan_create", C.byref(d), C.byref(plan))
        _spec_plans[key] = plan
    return plan


# Listeners for gradients the engine writes straight into the caller's storage (direct_grads): autograd never sees those
# tensors, so a data-parallel trainer that starts a gradient exchange as soon as a segment is complete
# (trainer.FlatGradBucket.enable_segmented_exchange) learns about them here.  Called with the list of written tensors.
DIRECT_WRITE_HOOKS = []


# Direct gradient writes are valid only when a parameter is used by exactly ONE engine call per step.  Models whose
# parameters may be reused (RNO2d over several time steps / predicted steps) run their forward under single_use(flag): with
# the flag off, `direct_grads` requests inside are ignored and autograd accumulates as usual (the bucket is zeroed in full
# for such models: FlatGradBucket(direct_module=..., zero_all=True)).
_SINGLE_USE = [True]
LAST_FORWARD_SINGLE_USE = [True]       # what the most recent declaring forward said (read by the gradient buckets: a parameter
                                       # used several times "arrives" several times, so segments must not leave early)


class single_use(object):
    def __init__(self, ok):
        self.ok = bool(ok)

    def __enter__(self):
        _SINGLE_USE.append(self.ok)
        LAST_FORWARD_SINGLE_USE[0] = self.ok

    def __exit__(self, *exc):
        _SINGLE_USE.pop()


def plane_major(w):
    """True when a corner weight (complex (Cin, Cout, m.., wl) or its real view (.., wl, 2)) is stored PLANE-MAJOR: the last
    mode dim outermost in memory, everything else contiguous behind it (include/fnoengine.h, weight_planes) - the layout
    libs.models.pino_models.basics.SpectralConv3d gives its parameters, so that the live last-dim slices are one
    contiguous prefix.  A tensor that is also contiguous in the ordinary sense (wl = 1) counts as ordinary."""
    r = torch.view_as_real(w) if w.is_complex() else w
    if r.dim() < 4 or r.is_contiguous() or r.stride(-1) != 1:
        return False
    plane = r[..., 0, :]
    return plane.is_contiguous() and r.stride(-2) == plane.numel()


def to_plane_major(w):
    """The same values with the last dim outermost in memory (shape unchanged)."""
    nd = w.dim()
    return w.permute(nd - 1, *range(nd - 1)).contiguous().permute(*range(1, nd), 0)


def _weights_ready(ws):
    """(tensors the engine can read in place, weight_planes flag): all plane-major -> as they are; otherwise contiguous"""
    if ws and all(plane_major(t) for t in ws):
        return list(ws), True
    return [t.contiguous() for t in ws], False


def _check_corner_weights(entry, ws, anchor, cin, cout, modes, last=None):
    """The front door for corner weights (real views): -> (tensors the engine reads in place, weight_planes flag).  Each goes
    through _operand in the layout _weights_ready settled.  A corner weight of the wrong extent is an out-of-bounds read on
    the device, not an error, so the shape must be (cin, cout, *modes, 2) - what the reference's einsum would have refused
    otherwise - with `last` (the stored last-dim extent of the standalone plans) in place of modes[-1] when given.  Without
    `last` (block stacks), plane-major weights carry their own extents: plane_major() has checked them against the strides."""
    ws, planes = _weights_ready(ws)
    want = None
    if last is not None or not planes:
        want = (int(cin), int(cout)) + tuple(int(m) for m in modes[:-1]) + (int(modes[-1] if last is None else last), 2)
    return [_operand(entry, f"spectral weight {i}", t, anchor, shape=want, layout="keep") for i, t in enumerate(ws)], planes


def _same_layout(g, w):
    return g is not None and g.shape == w.shape and g.stride() == w.stride() and (g.is_contiguous() or plane_major(g))


def _fresh_grads(ws, planes):
    """gradient tensors laid out like the weights; plane-major: zeros (the engine writes the live planes only)"""
    return [torch.zeros_like(t) if planes else torch.empty_like(t) for t in ws]


def _real_views(ws):
    return [torch.view_as_real(t) if t.is_complex() else t for t in ws]


def _direct_views(direct_grads, spec_ws, last_dim=None):
    """the weights' own .grad storage as real views, or None when direct writes are off / not possible.
    `last_dim` = the data's last extent: with plane-major weights the engine writes only the live planes
    [0, min(last_dim / 2 + 1, modes3)) of a gradient and nobody else clears a direct-write region (the bucket's zero()
    skips it), so when the live extent SHRINKS against the previous direct write the planes in between are cleared here -
    they would otherwise keep the last step's gradient (a batch with a shorter last dim behind a longer one)."""
    if not (direct_grads and _SINGLE_USE[-1] and torch.is_grad_enabled()
            and all(_same_layout(t.grad, t) for t in spec_ws)):
        return None
    if last_dim is not None:
        for t in spec_ws:
            if t.is_complex() and plane_major(t):
                k = min(int(last_dim) // 2 + 1, t.shape[-1])
                prev = t.__dict__.get("_fno_direct_k", 0)
                if k < prev:
                    t.grad[..., k:prev].zero_()
                t._fno_direct_k = k
    return [torch.view_as_real(t.grad) if t.grad.is_complex() else t.grad for t in spec_ws]


def _notify_direct(tensors):
    """DIRECT_WRITE_HOOKS holds weak references to bound methods (a bucket that went away must not be kept alive, nor
    polled): dead entries are dropped here."""
    dead = []
    for ref in DIRECT_WRITE_HOOKS:
        h = ref() if isinstance(ref, weakref.WeakMethod) else ref
        if h is None:
            dead.append(ref)
        else:
            h(tensors)
    for ref in dead:
        DIRECT_WRITE_HOOKS.remove(ref)


class _SpectralConvFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, bias, modes, norm, weight_last_extent, direct, *weights):
        e = "spectral_conv"
        _require_cuda(x, "x")
        x = x.contiguous()
        B, cin = x.shape[0], x.shape[1]
        dims = tuple(x.shape[2:])
        ndim = len(dims)
        if len(weights) != 2 ** (ndim - 1) or len(modes) != ndim:
            raise RuntimeError(f"fnoengine {e}: {len(weights)} corner weights / {len(modes)} mode counts for {ndim}-d data")
        cout = weights[0].shape[1]
        wl = int(weight_last_extent) if weight_last_extent else int(modes[-1])
        ws_list, planes = _check_corner_weights(e, weights, x, cin, cout, modes, last=wl)        # real views (.., 2)
        b = _operand(e, "bias", bias, x, numel=cout, optional=True)
        L = _lib.lib()
        plan = spec_plan(ndim, cin, cout, dims, modes, weight_last_extent, norm, x.device, weight_planes=planes)
        ctx.planes = planes
        y = torch.empty((B, cout) + dims, dtype=torch.float32, device=x.device)
        xhat = _bytes(L.fno_spec_xhat_bytes(plan, B), x.device)
        nws = L.fno_spec_workspace_bytes(plan, B)
        ws = _bytes(nws, x.device)
        _call("spec_forward", x.device, "fno_spec_forward", plan, B, x, _ptr_array(ws_list, 4), b, y, xhat, ws, nws, STREAM)
        ctx.plan, ctx.B, ctx.has_bias = plan, B, bias is not None
        ctx.x_shape = x.shape
        ctx.direct = direct
        ctx.save_for_backward(xhat, *ws_list)
        return y

    @staticmethod
    def backward(ctx, dy):
        xhat, *ws_list = ctx.saved_tensors
        dy = _operand("spectral_conv backward", "dy", dy, xhat)
        L = _lib.lib()
        need_dx = ctx.needs_input_grad[0]
        need_db = ctx.has_bias and ctx.needs_input_grad[1]
        need_dw = any(ctx.needs_input_grad[6:])
        dx = torch.empty(ctx.x_shape, dtype=torch.float32, device=dy.device) if need_dx else None
        direct = ctx.direct if need_dw else None
        dws = (direct if direct is not None else _fresh_grads(ws_list, ctx.planes)) if need_dw else None
        db = torch.empty(dy.shape[1], dtype=torch.float32, device=dy.device) if need_db else None
        nws = L.fno_spec_workspace_bytes(ctx.plan, ctx.B)
        ws = _bytes(nws, dy.device)
        _call("spec_backward", dy.device, "fno_spec_backward", ctx.plan, ctx.B, dy, xhat, _ptr_array(ws_list, 4), dx,
              _ptr_array(dws, 4), db, ws, nws, STREAM)
        if direct is not None:                     # written in place into the caller's gradient storage
            _notify_direct(direct)
            return (dx, db, None, None, None, None) + (None,) * len(ws_list)
        return (dx, db, None, None, None, None) + (tuple(dws) if need_dw else (None,) * len(ws_list))


def spectral_conv(x, weights, bias, modes, norm="backward", weight_last_extent=None, direct_grads=False):
    """y = irfftn(pad(W_c . rfftn(x)[corner_c]), s=x.shape[2:]) (+ bias[None, :, None..]).

    weights: corner tensors in canonical order, real (Cin, Cout, m.., 2) or complex.
    modes:   kept extent per corner along each dim.
    direct_grads: the backward WRITES dL/dW into the weights' existing contiguous `.grad` storage (e.g. views of a
    trainer.FlatGradBucket) instead of returning it to autograd: no accumulation kernel, no zeroing needed.  Only valid when
    each weight feeds exactly one spectral_conv call per step.
    """
    ws = _real_views(weights)
    wle = int(weight_last_extent) if weight_last_extent is not None else int(ws[0].shape[-2])
    b = bias.reshape(-1) if bias is not None else None
    direct = _direct_views(direct_grads, weights, last_dim=x.shape[-1])
    return _SpectralConvFn.apply(x, b, tuple(int(m) for m in modes), norm, wle, direct, *ws)
