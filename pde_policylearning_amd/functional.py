"""torch.autograd bridges onto the fnoengine C ABI.

PyTorch is plumbing here: it owns device memory (inputs, outputs, workspace, the
forward->backward stash) and the stream; all arithmetic happens in the HIP library.

The C ABI takes raw pointers and cannot see a tensor's device, dtype or extent, so this module is where they are checked.
Two helpers carry that ("The Python bridge"):
  _operand   every tensor passes through it before its address is taken: same device as the entry point's anchor (its first
             operand, itself through _require_cuda), the expected dtype, the stated extent; returns it contiguous.
  _call      every launching engine function is called through it: enters the anchor's device, reads the current stream
             there, turns tensors into addresses, calls, and raises on a non-zero return code.
Every forward / backward below reads: check operands, allocate, call.
"""
import ctypes as C
import functools
import math
import typing
import weakref

import torch

from . import _lib

_spec_plans = {}
_model_plans = {}
_Tensor = torch.Tensor


def _require_cuda(t, name):
    if not t.is_cuda:
        raise RuntimeError(f"fnoengine: `{name}` must live on the GPU (got {t.device}); "
                           "the engine has no CPU path")
    if t.dtype != torch.float32:
        raise RuntimeError(f"fnoengine: `{name}` must be float32 (got {t.dtype})")


def _bytes(n, device):
    return torch.empty(max(int(n), 256), dtype=torch.uint8, device=device)


def _refuse(entry, name, need, got):
    return RuntimeError(f"fnoengine {entry}: `{name}` must {need} (got {got}); refused before anything is launched")


def _operand(entry, name, t, anchor, dtype=torch.float32, numel=None, shape=None, optional=False, layout="copy"):
    """The one check between a tensor and its address.  `anchor`: the entry point's first operand (already through
    _require_cuda); only its device is read, so CPU tensors can drive this function in a test.  Returns the tensor
    contiguous (layout "copy": a copy when it is not), or None for an absent `optional` operand.  layout "dense": the engine
    writes the tensor in place, so it must be contiguous as it stands; "keep": returned as it is (corner weights, whose
    layout _weights_ready has settled).  Raises RuntimeError naming entry point, operand, what is needed and what was got."""
    if t is None:
        if optional:
            return None
        raise _refuse(entry, name, "be given", None)
    if t.device != anchor.device:
        raise _refuse(entry, name, f"live on {anchor.device}, the GPU of the call's first operand", t.device)
    if t.dtype != dtype:
        raise _refuse(entry, name, f"be {dtype}", t.dtype)
    if numel is not None and t.numel() != numel:
        raise _refuse(entry, name, f"have {numel} elements", f"{t.numel()}, shape {tuple(t.shape)}")
    if shape is not None and t.shape != shape:
        raise _refuse(entry, name, f"have shape {tuple(shape)}", tuple(t.shape))
    if layout == "copy":
        return t.contiguous()
    if layout == "dense" and not t.is_contiguous():
        raise _refuse(entry, name, "be contiguous (it is written in place)", f"strides {t.stride()}")
    return t


STREAM = object()       # stands for the current stream in _call's argument list (it is not always the last argument)


def _ptr(t):
    """address of a tensor that has been through _operand (None: NULL)"""
    return None if t is None else t.data_ptr()


def _call(what, device, fname, *args):
    """The one way into a launching engine function: on `device` (the anchor's), with the stream current THERE in place of
    STREAM and tensors / None as addresses / NULL; a non-zero return code raises with the library's message."""
    with torch.cuda.device(device):
        stream = torch.cuda.current_stream().cuda_stream
        rc = getattr(_lib.lib(), fname)(*[stream if a is STREAM else a.data_ptr() if isinstance(a, _Tensor) else a
                                          for a in args])
    _lib.check(rc, what)


def _ptr_array(tensors, slots=None):
    """void*[slots] over checked tensors, NULL-filled (None: NULL); slots = 4 is the corner-weight array of fno_spec_*"""
    if tensors is None:
        return None
    slots = len(tensors) if slots is None else slots
    return (C.c_void_p * slots)(*[t.data_ptr() for t in tensors] + [0] * (slots - len(tensors)))


def _plan_available(cache, key, create, *args):
    """True when `create(*args)` (a plan constructor) accepts the configuration; cached under `key`.  An unsupported shape is
    not an error for callers that have another path."""
    ok = cache.get(key)
    if ok is None:
        try:
            create(*args)
            ok = True
        except RuntimeError:
            ok = False
        cache[key] = ok
    return ok


# ----------------------------------------------------------------------------
# shape rules, each stated once
# ----------------------------------------------------------------------------
def plane_size(shape):
    """elements per (batch, channel) plane of a (B, C, ...) shape"""
    return math.prod(shape[2:])


def gemm_mode():
    """the engine's channel-GEMM mode: 1 split precision (default), 0 exact fp32 (include/fnoengine.h, fno_set_gemm_mode)"""
    return _lib.lib().fno_get_gemm_mode()


def row_tiling(dims, mode=None):
    """How the fused block kernels cover a grid `dims`: "tiled" - rows of 32 / 64 / 128 / 256 floats that tile the 128-pixel
    (256 for rows above 128) workgroup tile, planes a multiple of the tile; "loose" - any other last dim in 32..320 on planes
    that tile by 128 pixels (the PINO observers' padded time axis 73, 96 x 96, 160 x 160): tiles of the flattened plane,
    spectral rows gathered per tile, split-precision GEMM mode only (`mode`, default: the engine's current one); else None.
    The engine keeps the last word (fno_model_plan_create: tile + twiddle tables must fit LDS)."""
    w, pw = dims[-1], math.prod(dims)
    npx = 256 if w > 128 else 128
    if w % 32 == 0 and w <= 256 and npx % w == 0 and pw % npx == 0:
        return "tiled"
    if 32 <= w <= 320 and pw % 128 == 0 and (gemm_mode() if mode is None else mode) == 1:
        return "loose"
    return None


def default_gelu_mask(n_layers):
    """bit l set = GELU after layer l: the reference applies it while l < n_layers - l (fno_block.py:149)"""
    return sum(1 << l for l in range(n_layers) if l < n_layers - l)


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


# ----------------------------------------------------------------------------
# fused FNO model
# ----------------------------------------------------------------------------
def model_plan(ndim, cin, c, cout, hidden_proj, n_layers, dims, modes, norm, gelu_mask, device, weight_planes=False):
    key = (ndim, cin, c, cout, hidden_proj, n_layers, tuple(dims), tuple(modes), norm, gelu_mask, device.index) \
        + ((True,) if weight_planes else ())
    plan = _model_plans.get(key)
    if plan is None:
        d = _lib.FnoModelDesc()
        d.ndim, d.Cin, d.C, d.Cout = ndim, cin, c, cout
        d.hidden_proj, d.n_layers = hidden_proj, n_layers
        for i in range(ndim):
            d.dims[i], d.modes[i] = int(dims[i]), int(modes[i])
        d.norm = _lib.NORM_CODES[norm]
        d.gelu_mask = gelu_mask
        d.weight_planes = 1 if weight_planes else 0
        plan = C.c_void_p()
        _call("model_plan_create", device, "fno_model_plan_create", C.byref(d), C.byref(plan))
        _model_plans[key] = plan
    return plan


def model_plan_available(ndim, cin, c, cout, hidden_proj, n_layers, dims, modes, norm, gelu_mask, device):
    """True when fno_model_plan_create accepts the configuration (result cached; an unsupported shape is not an error
    for callers that have an unfused path)."""
    key = ("avail", ndim, cin, c, cout, hidden_proj, n_layers, tuple(dims), tuple(modes), norm, gelu_mask, device.index)
    return _plan_available(_model_plans, key, model_plan, ndim, cin, c, cout, hidden_proj, n_layers, dims, modes, norm,
                           gelu_mask, device)


_ENDS = ("lift_w", "lift_b", "w1", "b1", "w2", "b2")        # the model's parameters outside the block stack, in ABI order


class _FNOModelFn(torch.autograd.Function):
    """Whole FNO forward/backward in the HIP engine.  Tensor arguments, in order:
    x, lift_w, lift_b, spec_bias (or None), w1, b1, w2, b2, skip_w[0..L), spec_w[0..L*ncorner)."""

    @staticmethod
    def forward(ctx, cfg, x, lift_w, lift_b, spec_bias, w1, b1, w2, b2, *rest):
        e = "fno_model"
        n_layers, modes, norm, gelu_mask, direct, overlap, _ = cfg
        ctx.direct = direct
        ctx.overlap = overlap
        _require_cuda(x, "x")
        x = x.contiguous()
        dims = tuple(x.shape[2:])
        ndim = len(dims)
        ncorner = 2 ** (ndim - 1)
        assert len(rest) == n_layers + n_layers * ncorner
        B, cin = x.shape[0], x.shape[1]
        c, cout, hid = lift_w.shape[0], w2.shape[0], w1.shape[0]
        ends = [_operand(e, nm, t, x, numel=n) for nm, t, n in (
            ("lifting weight", lift_w, c * cin), ("lifting bias", lift_b, c), ("projection W1", w1, hid * c),
            ("projection b1", b1, hid), ("projection W2", w2, cout * hid), ("projection b2", b2, cout))]
        skip_ws = [_operand(e, f"skip weight {l}", t, x, numel=c * c) for l, t in enumerate(rest[:n_layers])]
        want = (c, c) + tuple(modes) + (2,)             # the whole model takes contiguous corner weights only
        spec_ws = [_operand(e, f"spectral weight {i}", t, x, shape=want) for i, t in enumerate(rest[n_layers:])]
        sb = _operand(e, "spectral bias", spec_bias, x, numel=n_layers * c, optional=True)
        if direct is not None:          # gradient storage the backward writes in place: one tensor per parameter, same extent
            pairs = list(zip(ends, (direct[k] for k in _ENDS))) + list(zip(skip_ws, direct["skip"])) \
                + list(zip(spec_ws, direct["spec"])) + ([(sb, direct["spec_bias"])] if sb is not None else [])
            for p, g in pairs:
                _operand(e, "direct-write gradient", g, x, numel=p.numel(), layout="dense")
        L = _lib.lib()
        plan = model_plan(ndim, cin, c, cout, hid, n_layers, dims, modes, norm, gelu_mask, x.device)
        prm = _fill_params(ncorner, skip_ws, spec_ws, sb, ends)
        y = torch.empty((B, cout) + dims, dtype=torch.float32, device=x.device)
        saved = _bytes(L.fno_model_saved_bytes(plan, B), x.device)
        nws = L.fno_model_workspace_bytes(plan, B)
        ws = _bytes(nws, x.device)
        _call("model_forward", x.device, "fno_model_forward", plan, B, C.byref(prm), x, y, saved, ws, nws, STREAM)
        ctx.plan, ctx.B, ctx.n_layers, ctx.ncorner = plan, B, n_layers, ncorner
        ctx.has_sb = sb is not None
        ctx.save_for_backward(x, saved, *ends, *skip_ws, *spec_ws, *([sb] if sb is not None else []))
        return y

    @staticmethod
    def backward(ctx, dy):
        sv = ctx.saved_tensors
        x, saved = sv[:2]
        ends = sv[2:8]
        nl, nc = ctx.n_layers, ctx.ncorner
        skip_ws, spec_ws, sb = _saved_params(sv, 8, nl, nc, ctx.has_sb)
        dy = _operand("fno_model backward", "dy", dy, x)
        L = _lib.lib()
        prm = _fill_params(nc, skip_ws, spec_ws, sb, ends)
        if ctx.direct is not None:
            # the engine WRITES gradients: hand it the parameters' own (pre-allocated, flat-bucket)
            # .grad storage and return None so autograd launches no accumulation kernels
            dg = ctx.direct
            g = [dg[k] for k in _ENDS]
            g_skip, g_spec, g_sb = dg["skip"], dg["spec"], dg["spec_bias"]
        else:
            g = [torch.empty_like(t) for t in ends]
            g_skip = [torch.empty_like(t) for t in skip_ws]
            g_spec = [torch.empty_like(t) for t in spec_ws]
            g_sb = torch.empty_like(sb) if sb is not None else None
        grd = _fill_params(nc, g_skip, g_spec, g_sb, g, _lib.FnoModelGrads)
        nws = L.fno_model_workspace_bytes(ctx.plan, ctx.B)
        ws = _bytes(nws, dy.device)
        ov = ctx.overlap
        # dL/dx through the lifting layer (run_control.py:186-224 differentiates the observer down to its input field)
        dx = torch.empty_like(x) if ctx.needs_input_grad[1] else None
        common = (ctx.plan, ctx.B, C.byref(prm), x, dy, saved, C.byref(grd))
        if dx is not None:
            _call("model_backward_dx", dy.device, "fno_model_backward_dx", *common, dx, ws, nws, STREAM)
        elif ov is not None and ctx.direct is not None and 0 < ov.split_layer < nl:
            # late layers first; their finished gradients go on the wire while the early layers are differentiated
            k = ov.split_layer
            _call("model_backward_part", dy.device, "fno_model_backward_part", *common, None, ws, nws, STREAM, nl - 1, k)
            ov.late_gradients_ready()
            _call("model_backward_part", dy.device, "fno_model_backward_part", *common, None, ws, nws, STREAM, k - 1, 0)
        else:
            _call("model_backward", dy.device, "fno_model_backward", *common, ws, nws, STREAM)
        if ctx.direct is not None:
            return (None, dx) + (None,) * (7 + len(skip_ws) + len(spec_ws))
        return (None, dx, g[0], g[1], g_sb, g[2], g[3], g[4], g[5]) + tuple(g_skip) + tuple(g_spec)


def fno_model(x, lift_w, lift_b, skip_ws, spec_ws, spec_bias, w1, b1, w2, b2, modes, norm="forward",
              gelu_mask=None, direct_grads=False, overlap=None):
    """Fused neuralop.models.FNO forward (default configuration).  `modes` = kept per
    corner per dim (n_modes // 2); `spec_ws` real-view corner weights, layer-major."""
    n_layers = len(skip_ws)
    if gelu_mask is None:
        gelu_mask = default_gelu_mask(n_layers)
    direct = None
    if direct_grads:
        params = [lift_w, lift_b, w1, b1, w2, b2] + list(skip_ws) + list(spec_ws) + ([spec_bias] if spec_bias is not None else [])
        if all(p.grad is not None and p.grad.is_contiguous() for p in params):
            direct = dict(lift_w=lift_w.grad, lift_b=lift_b.grad, w1=w1.grad, b1=b1.grad, w2=w2.grad, b2=b2.grad,
                          skip=[p.grad for p in skip_ws], spec=[p.grad for p in spec_ws],
                          spec_bias=spec_bias.grad if spec_bias is not None else None)
    cfg = _Cfg(n_layers, tuple(int(m) for m in modes), norm, int(gelu_mask), direct, overlap if direct is not None else None)
    return _FNOModelFn.apply(cfg, x, lift_w, lift_b, spec_bias, w1, b1, w2, b2, *skip_ws, *spec_ws)


# ----------------------------------------------------------------------------
# training-step tail: decode + relative-L2 loss, Adam on a flat bucket
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


def _adam_state(e, param, grad, exp_avg, exp_avg_sq, step_counter, scratch, compact=False):
    """the buffers of an Adam update (all updated or read in place: dense, never copied); compact: the moments have a
    size of their own (adam_step_runs)"""
    _require_cuda(param, "param")
    _operand(e, "grad", grad, param, numel=param.numel(), layout="dense")
    _operand(e, "param", param, param, layout="dense")
    _operand(e, "exp_avg", exp_avg, param, numel=None if compact else param.numel(), layout="dense")
    _operand(e, "exp_avg_sq", exp_avg_sq, param, numel=exp_avg.numel(), layout="dense")
    if step_counter is not None:
        _operand(e, "step_counter", step_counter, param, dtype=torch.int32, numel=1, layout="dense")
        _operand(e, "scratch", scratch, param, numel=2, layout="dense")


def adam_step(param, grad, exp_avg, exp_avg_sq, step, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0,
              step_counter=None, scratch=None):
    """One torch.optim.Adam update of a flat fp32 bucket, in place, one kernel.  With `step_counter`
    (int32 device tensor) the step count lives on the device (fno_adam_step_dev: graph-replayable)."""
    _adam_state("adam_step", param, grad, exp_avg, exp_avg_sq, step_counter, scratch)
    hp = (float(lr), float(betas[0]), float(betas[1]), float(eps), float(weight_decay))
    if step_counter is not None:
        _call("adam_step_dev", param.device, "fno_adam_step_dev", param.numel(), param, grad, exp_avg, exp_avg_sq, *hp,
              step_counter, scratch, STREAM)
        return
    _call("adam_step", param.device, "fno_adam_step", param.numel(), param, grad, exp_avg, exp_avg_sq, *hp, int(step), STREAM)


def adam_step_runs(runs, param, grad, exp_avg, exp_avg_sq, step, lr, betas, eps, weight_decay, step_counter=None,
                   scratch=None):
    """One Adam update of a bucket planned around dead last-dim slices (trainer.FusedAdam.skip_dead_slices): `runs` lists
    ("dense", offset, n, compact offset) ranges and ("rows", offset, rows, row_len, live_len, compact offset) blocks of
    `param` / `grad` (full layout); exp_avg / exp_avg_sq are compact.  One kernel per run, the dead part of a block untouched."""
    _adam_state("adam_step_runs", param, grad, exp_avg, exp_avg_sq, step_counter, scratch, compact=True)
    dev = param.device
    if step_counter is not None:
        _call("adam_prep_dev", dev, "fno_adam_prep_dev", step_counter, scratch, float(lr), float(betas[0]), float(betas[1]),
              STREAM)
    hp = (float(lr), float(betas[0]), float(betas[1]), float(eps), float(weight_decay), int(step))
    dyn = scratch if step_counter is not None else None
    # addresses of the runs inside the four checked buffers: each run is held against the buffers' extents below
    P, G, M, V = param.data_ptr(), grad.data_ptr(), exp_avg.data_ptr(), exp_avg_sq.data_ptr()
    for run in runs:
        if run[0] == "dense":
            _, off, n, coff = run
            if off < 0 or coff < 0 or off + n > param.numel() or coff + n > exp_avg.numel():
                raise RuntimeError("fnoengine adam_step_runs: run outside the buffers")
            _call("adam_step_range", dev, "fno_adam_step_range", n, P + 4 * off, G + 4 * off, M + 4 * coff, V + 4 * coff, *hp,
                  dyn, STREAM)
        else:
            _, off, rows, row_len, live_len, coff = run
            if off < 0 or coff < 0 or off + rows * row_len > param.numel() or coff + rows * live_len > exp_avg.numel():
                raise RuntimeError("fnoengine adam_step_runs: block outside the buffers")
            _call("adam_step_live", dev, "fno_adam_step_live", rows, row_len, live_len, P + 4 * off, G + 4 * off, M + 4 * coff,
                  V + 4 * coff, *hp, dyn, STREAM)


def adam_replay_scalars(step_from, nsteps, lr, betas, device, on_device=False):
    """(2 * nsteps,) device tensor: {lr / (1 - beta1^t), sqrt(1 - beta2^t)} for t = step_from .. step_from + nsteps - 1,
    derived as the stepping kernels' callers derive them: on the host in double (fno_adam_step), or - on_device - by the
    device arithmetic of the graph-replayable path (fno_adam_step_dev)."""
    if on_device:
        scal = torch.empty(2 * nsteps, dtype=torch.float32, device=device)
        _call("adam_replay_prep", device, "fno_adam_replay_prep", scal, int(step_from), int(nsteps), float(lr), float(betas[0]),
              float(betas[1]), STREAM)
        return scal
    host = torch.empty(2 * nsteps, dtype=torch.float32)
    base = host.data_ptr()                      # host memory, host-only call: nothing crosses to the device here
    for j in range(nsteps):
        _lib.lib().fno_adam_scalars(float(lr), float(betas[0]), float(betas[1]), int(step_from + j), C.c_void_p(base + 8 * j))
    return host.to(device)


def adam_replay_dead(rows, row_len, live_len, param_block, dead_m, dead_v, moments_zero, scal, betas, eps, weight_decay):
    """Take the dead part of a row-sliced block (rows x row_len floats of `param_block`, dead = [live_len, row_len) of each
    row) through the Adam steps described by `scal` (adam_replay_scalars) with a zero gradient; dead_m / dead_v: compact
    dead moments, read unless moments_zero, always written."""
    e = "adam_replay_dead"
    _require_cuda(param_block, "param")
    nd = rows * (row_len - live_len)
    for t, name, n in ((param_block, "param", rows * row_len), (dead_m, "dead exp_avg", nd), (dead_v, "dead exp_avg_sq", nd),
                       (scal, "scalars", None)):
        _operand(e, name, t, param_block, numel=n, layout="dense")
    if scal.numel() % 2:
        raise RuntimeError(f"fnoengine {e}: `scalars` holds two floats per step (got {scal.numel()} elements)")
    _call(e, param_block.device, "fno_adam_replay_dead", rows, row_len, live_len, param_block, dead_m, dead_v,
          1 if moments_zero else 0, scal, scal.numel() // 2, float(betas[0]), float(betas[1]), float(eps), float(weight_decay),
          STREAM)


# ----------------------------------------------------------------------------
# fused block stack: y = B_{L-1}(...B_0(x)),  B_l(u) = [gelu](specconv_l(u) + conv1x1_l(u) + bias_l)
# ----------------------------------------------------------------------------
def _block_tail(relu_out, drop_p, seed, y):
    """FnoBlockTail over checked tensors (seed: two int32 words on the device; y: the forward's output, backward only)"""
    return _lib.FnoBlockTail(int(relu_out), float(drop_p), _ptr(seed), _ptr(y))


class _FNOBlocksFn(torch.autograd.Function):
    """Tensor arguments: x, bias (L, C) or None, skip_w[0..L), spec_w[0..L*ncorner)."""

    @staticmethod
    def forward(ctx, cfg, x, bias, *rest):
        n_layers, modes, norm, gelu_mask, direct, _, tail = cfg      # tail: fno_model_*_tail
        e = "fno_blocks" if tail is None else "fno_block_tail"
        ctx.direct = direct
        _require_cuda(x, "x")
        x = x.contiguous()
        dims = tuple(x.shape[2:])
        ndim = len(dims)
        ncorner = 2 ** (ndim - 1)
        assert len(rest) == n_layers + n_layers * ncorner
        B, c = x.shape[0], x.shape[1]
        skip_ws = [_operand(e, f"skip weight {l}", t, x, numel=c * c) for l, t in enumerate(rest[:n_layers])]
        spec_ws, planes = _check_corner_weights(e, rest[n_layers:], x, c, c, modes)
        ctx.planes = planes
        sb = _operand(e, "bias", bias, x, numel=n_layers * c, optional=True)
        seed = None if tail is None else _operand(e, "seed", tail[2], x, dtype=torch.int32, numel=2, optional=True)
        L = _lib.lib()
        plan = model_plan(ndim, 0, c, 0, 0, n_layers, dims, modes, norm, gelu_mask, x.device, weight_planes=planes)
        prm = _fill_params(ncorner, skip_ws, spec_ws, sb)
        y = torch.empty_like(x)
        saved = _bytes(L.fno_model_saved_bytes(plan, B), x.device)
        nws = L.fno_model_workspace_bytes(plan, B)
        ws = _bytes(nws, x.device)
        if tail is None:
            _call("blocks_forward", x.device, "fno_model_forward", plan, B, C.byref(prm), x, y, saved, ws, nws, STREAM)
        else:
            t = _block_tail(tail[0], tail[1], seed, None)
            _call("blocks_forward_tail", x.device, "fno_model_forward_tail", plan, B, C.byref(prm), x, y, saved, ws, nws, STREAM,
                  C.byref(t))
        ctx.plan, ctx.B, ctx.n_layers, ctx.ncorner, ctx.has_sb = plan, B, n_layers, ncorner, sb is not None
        ctx.tail = None if tail is None else (bool(tail[0]), float(tail[1]))
        extra = []
        if tail is not None:
            extra = [y if tail[0] else x.new_empty(0), seed if seed is not None else x.new_empty(0)]
        ctx.save_for_backward(x, saved, *skip_ws, *spec_ws, *([sb] if sb is not None else []), *extra)
        return y

    @staticmethod
    def backward(ctx, dy):
        sv = ctx.saved_tensors
        x, saved = sv[:2]
        nl, nc = ctx.n_layers, ctx.ncorner
        skip_ws, spec_ws, sb = _saved_params(sv, 2, nl, nc, ctx.has_sb)
        dy = _operand("fno_blocks backward", "dy", dy, x)
        L = _lib.lib()
        g_skip = [torch.empty_like(t) for t in skip_ws]
        g_spec = ctx.direct if ctx.direct is not None else _fresh_grads(spec_ws, ctx.planes)   # direct: the weights' own .grad storage
        g_sb = torch.empty_like(sb) if sb is not None else None
        prm, grd = _fill_params(nc, skip_ws, spec_ws, sb), _fill_params(nc, g_skip, g_spec, g_sb, struct=_lib.FnoModelGrads)
        dx = torch.empty_like(x) if ctx.needs_input_grad[1] else None
        nws = L.fno_model_workspace_bytes(ctx.plan, ctx.B)
        ws = _bytes(nws, dy.device)
        common = (ctx.plan, ctx.B, C.byref(prm), x, dy, saved, C.byref(grd), dx, ws, nws, STREAM)
        if ctx.tail is None:
            _call("blocks_backward", dy.device, "fno_model_backward_dx", *common)
        else:
            y_out, seed = sv[-2], sv[-1]
            t = _block_tail(ctx.tail[0], ctx.tail[1], seed if seed.numel() else None, y_out if y_out.numel() else None)
            _call("blocks_backward_tail", dy.device, "fno_model_backward_tail", *common, C.byref(t))
        if ctx.direct is not None:
            _notify_direct(ctx.direct)
        return (None, dx, g_sb) + tuple(g_skip) + ((None,) * len(g_spec) if ctx.direct is not None else tuple(g_spec))


def blocks_supported(x, n_layers=1, modes=None, norm="backward", gelu_mask=0):
    """Shapes the fused block kernels cover (fno_model_plan_create): 32 / 64 channels and a grid row_tiling() covers; with
    `modes` the engine itself is asked (tile + twiddle tables must fit LDS)."""
    if not (x.is_cuda and x.dtype == torch.float32 and x.dim() in (4, 5)):
        return False
    c = x.shape[1]
    if not (c in (32, 64) and row_tiling(x.shape[2:]) is not None and n_layers <= _lib.FNO_MAX_LAYERS):
        return False
    if modes is None:
        return True
    return model_plan_available(x.dim() - 2, 0, c, 0, 0, n_layers, tuple(x.shape[2:]), tuple(int(m) for m in modes), norm,
                                int(gelu_mask), x.device)


def block_tail_supported(x, modes, norm):
    """Shapes fno_block_tail covers: what one fused block covers on whole rows (32 / 64 channels, rows of 32 / 64 / 128
    floats tiling 128-pixel tiles), in either GEMM mode."""
    if not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 4):
        return False
    if not (x.shape[1] in (32, 64) and x.shape[-1] in (32, 64, 128) and plane_size(x.shape) % 128 == 0):
        return False
    return blocks_supported(x, 1, modes, norm)


def draw_dropout_seed(device):
    """Two 32-bit words for the engine's counter-based dropout, drawn on the device by torch's generator: follows
    torch.manual_seed, and is safe under hipGraph capture (the generator's offset advances per replay)."""
    return torch.randint(-2 ** 31, 2 ** 31 - 1, (2,), device=device, dtype=torch.int32)


def dropout_scale(n, drop_p, seed, device):
    """The 0 / 1/(1-p) field the kernels regenerate from `seed` for a tensor of n elements (tests, oracles)."""
    out = torch.empty(n, dtype=torch.float32, device=device)
    seed = _operand("dropout_scale", "seed", seed, out, dtype=torch.int32, numel=2, optional=True)
    _call("dropout_scale", device, "fno_dropout_scale", n, float(drop_p), seed, out, STREAM)
    return out


def fno_block_tail(x, skip_w, spec_ws, bias, modes, norm, relu_out=True, drop_p=0.0, seed=None, direct_grads=False):
    """One fused Fourier layer with the tail of the RNO regressor's layers (rno.py:92-106, channels-first):
    y = relu(specconv(drop(x)) + skip_w x + bias).  `seed`: draw_dropout_seed() (required when drop_p > 0).  The ReLU, its
    derivative, the dropout mask (regenerated in the backward) and the accumulation of the two branches' input gradients
    all happen inside the engine kernels (fno_model_forward_tail / fno_model_backward_tail)."""
    direct = _direct_views(direct_grads, spec_ws)
    if drop_p > 0 and seed is None:
        raise ValueError("fno_block_tail: drop_p > 0 needs a seed (draw_dropout_seed)")
    cfg = _Cfg(1, tuple(int(m) for m in modes), norm, 0, direct,
               tail=(bool(relu_out), float(drop_p), seed if drop_p > 0 else None))
    return _FNOBlocksFn.apply(cfg, x, bias, skip_w, *_real_views(spec_ws))


def fno_blocks(x, skip_ws, spec_ws, bias, modes, norm, gelu_mask=0, direct_grads=False):
    """Stack of fused Fourier layers (include/fnoengine.h, block stacks): per layer one spectral
    convolution (corner weights `spec_ws`, layer-major, real view (C, C, m.., 2)), one 1x1 convolution
    (`skip_ws[l]`, (C, C) or (C, C, 1..)) and one bias row of `bias` (L, C); GELU after layer l iff bit l
    of `gelu_mask`.  Returns (B, C, ...); differentiable w.r.t. x and every parameter."""
    direct = _direct_views(direct_grads, spec_ws, last_dim=x.shape[-1])       # backward WRITES dL/dW of the spectral weights into their existing .grad storage
    cfg = _Cfg(len(skip_ws), tuple(int(m) for m in modes), norm, int(gelu_mask), direct)
    return _FNOBlocksFn.apply(cfg, x, bias, *skip_ws, *_real_views(spec_ws))


# ----------------------------------------------------------------------------
# fan-out of Fourier layers over one input (RNO cell: f1, f3, f5, f7 on x; f2, f4, f8 on h)
# ----------------------------------------------------------------------------
FANOUT_MAX = 4


class _FourierFanoutFn(torch.autograd.Function):
    """Tensor arguments: x, then skip_w[n], bias[n], spec_w[n * ncorner] (member-major).  Returns n tensors."""

    @staticmethod
    def forward(ctx, cfg, x, *rest):
        e = "fourier_fanout"
        n, modes, norm = cfg.n_layers, cfg.modes, cfg.norm
        ctx.direct = cfg.direct
        _require_cuda(x, "x")
        x = x.contiguous()
        dims = tuple(x.shape[2:])
        ndim = len(dims)
        nc = 2 ** (ndim - 1)
        assert len(rest) == 2 * n + n * nc and n <= FANOUT_MAX
        B, c = x.shape[0], x.shape[1]
        skip_ws = [_operand(e, f"skip weight {j}", t, x, numel=c * c) for j, t in enumerate(rest[:n])]
        biases = [_operand(e, f"bias {j}", t, x, numel=c) for j, t in enumerate(rest[n:2 * n])]
        spec_ws, planes = _check_corner_weights(e, rest[2 * n:], x, c, c, modes)
        ctx.planes = planes
        L = _lib.lib()
        plan = model_plan(ndim, 0, c, 0, 0, FANOUT_MAX, dims, modes, norm, 0, x.device, weight_planes=planes)
        prm = _fill_params(nc, skip_ws, spec_ws)
        ys = [torch.empty_like(x) for _ in range(n)]
        saved = _bytes(L.fno_fanout_saved_bytes(plan, B, n), x.device)
        nws = L.fno_fanout_workspace_bytes(plan, B, n)
        ws = _bytes(nws, x.device)
        _call("fanout_forward", x.device, "fno_fanout_forward", plan, B, n, C.byref(prm), _ptr_array(biases), x, _ptr_array(ys),
              saved, ws, nws, STREAM)
        ctx.plan, ctx.B, ctx.n, ctx.nc = plan, B, n, nc
        ctx.save_for_backward(x, saved, *skip_ws, *spec_ws)
        ctx.bias_shapes = [b.shape for b in rest[n:2 * n]]
        return tuple(ys)

    @staticmethod
    def backward(ctx, *dys):
        sv = ctx.saved_tensors
        x, saved = sv[:2]
        n, nc = ctx.n, ctx.nc
        skip_ws, spec_ws, _ = _saved_params(sv, 2, n, nc)
        dys = [torch.zeros_like(x) if d is None else _operand("fourier_fanout backward", "dy", d, x, numel=x.numel()) for d in dys]
        L = _lib.lib()
        g_skip = [torch.empty_like(t) for t in skip_ws]
        g_spec = ctx.direct if ctx.direct is not None else _fresh_grads(spec_ws, ctx.planes)     # direct: the weights' own .grad storage
        g_bias = [torch.empty(x.shape[1], dtype=torch.float32, device=x.device) for _ in range(n)]
        prm, grd = _fill_params(nc, skip_ws, spec_ws), _fill_params(nc, g_skip, g_spec, struct=_lib.FnoModelGrads)
        dx = torch.empty_like(x)
        nws = L.fno_fanout_workspace_bytes(ctx.plan, ctx.B, n)
        ws = _bytes(nws, x.device)
        _call("fanout_backward", x.device, "fno_fanout_backward", ctx.plan, ctx.B, n, C.byref(prm), x, _ptr_array(dys), saved,
              C.byref(grd), _ptr_array(g_bias), dx, ws, nws, STREAM)
        g_bias = [g.view(sh) for g, sh in zip(g_bias, ctx.bias_shapes)]
        if ctx.direct is not None:
            _notify_direct(ctx.direct)
        return ((None, dx if ctx.needs_input_grad[1] else None) + tuple(g_skip) + tuple(g_bias)
                + ((None,) * len(g_spec) if ctx.direct is not None else tuple(g_spec)))


def fanout_supported(x, n, modes, norm):
    if not (1 <= n <= FANOUT_MAX and blocks_supported(x)):
        return False
    return model_plan_available(x.dim() - 2, 0, x.shape[1], 0, 0, FANOUT_MAX, tuple(x.shape[2:]), tuple(int(m) for m in modes),
                                norm, 0, x.device)


def fourier_fanout(x, skip_ws, biases, spec_ws, modes, norm, direct_grads=False):
    """[SpecConv_j(x) + conv1x1(x; skip_ws[j]) + biases[j] for j < n]: n <= 4 Fourier layers (rno.py:215-228) on ONE input,
    whose forward transforms run once and whose input gradients are summed inside the backward kernels
    (include/fnoengine.h, fno_fanout_*).  spec_ws is member-major: member j's corner weights at [j * ncorner, (j+1) * ncorner)."""
    cfg = _Cfg(len(skip_ws), tuple(int(m) for m in modes), norm, 0, _direct_views(direct_grads, spec_ws))
    return _FourierFanoutFn.apply(cfg, x, *skip_ws, *biases, *spec_ws)


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
        gi = _operand("pino_loss backward", "g_ic", g_ic.contiguous().to(torch.float32), u_c, numel=1).reshape(1)
        gf = _operand("pino_loss backward", "g_f", g_f.contiguous().to(torch.float32), u_c, numel=1).reshape(1)
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
    if u.dim() == 4 and u.shape[-1] == 1:
        u = u[..., 0]
    if u.dim() != 3:
        raise RuntimeError(f"fnoengine {e}: `u` must be (B, nt, nx) or (B, nt, nx, 1) (got {tuple(u.shape)})")
    return u


def burgers_loss_supported(u):
    """the shapes k_burgers_loss.h takes: float32 on the GPU, (B, nt, nx[, 1]) with nt >= 3 and nx in BURGERS_NX"""
    if u.dim() == 4 and u.shape[-1] == 1:
        u = u[..., 0]
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
        gu = _operand("burgers_loss backward", "g_u", g_u.contiguous().to(torch.float32), u_c, numel=1).reshape(1)
        gf = _operand("burgers_loss backward", "g_f", g_f.contiguous().to(torch.float32), u_c, numel=1).reshape(1)
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
    if t.dim() == 4 and t.shape[-1] == 1:
        t = t[..., 0]
    if t.dim() != 3 or t.shape[1] != t.shape[2]:
        raise RuntimeError(f"fnoengine {e}: `{name}` must be (B, S, S) or (B, S, S, 1) on a square grid (got {tuple(t.shape)})")
    return t


def darcy_loss_supported(u):
    """the shapes k_darcy_loss.h takes: float32 on the GPU, (B, S, S[, 1]) with DARCY_S_MIN <= S <= DARCY_S_MAX"""
    if u.dim() == 4 and u.shape[-1] == 1:
        u = u[..., 0]
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
        gd = _operand(e, "g_data", g_data.contiguous().to(torch.float32), u_c, numel=1).reshape(1) if has_y else None
        gf = _operand(e, "g_f", g_f.contiguous().to(torch.float32), u_c, numel=1).reshape(1)
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


# ----------------------------------------------------------------------------
# channel-flow RHS and the physics-informed loss (libs/envs/control_env.py:429-530, 627-633)
# ----------------------------------------------------------------------------
class ChannelGrid:
    """The staggered channel grid the kernels need: sizes, uniform spacings dx, dz, viscosity nu and the wall-normal
    metrics y (Ny faces), ym (Ny-1 centres), yg (Ny+1 ghost-extended centres).  Packs the reciprocal spacings once on the
    host (fno_chanflow_pack_metrics) and keeps one device copy per GPU."""

    def __init__(self, Nx, Nz, dx, dz, y, ym, yg, nu):
        import numpy as np
        y, ym, yg = (np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(-1)) for a in (y, ym, yg))
        self.Nx, self.Ny, self.Nz = int(Nx), int(y.shape[0]), int(Nz)
        if ym.shape[0] != self.Ny - 1 or yg.shape[0] != self.Ny + 1:
            raise ValueError(f"channel grid: y has {self.Ny} faces, so ym needs {self.Ny - 1} and yg {self.Ny + 1} entries "
                             f"(got {ym.shape[0]}, {yg.shape[0]})")
        self.dx, self.dz, self.nu = float(dx), float(dz), float(nu)
        self.y, self.ym, self.yg = y, ym, yg
        self._packed = None
        self._dev = {}

    def desc(self):
        return _lib.FnoChanflowGrid(self.Nx, self.Ny, self.Nz, self.dx, self.dz, self.nu)

    def metrics(self, device):
        import numpy as np
        if self._packed is None:
            packed = np.zeros(3 * (self.Ny + 2), dtype=np.float64)
            dp = C.POINTER(C.c_double)
            _lib.check(_lib.lib().fno_chanflow_pack_metrics(self.Ny, self.y.ctypes.data_as(dp), self.ym.ctypes.data_as(dp),
                                                            self.yg.ctypes.data_as(dp), packed.ctypes.data_as(dp)),
                       "chanflow_pack_metrics")
            self._packed = packed
        if device not in self._dev:
            self._dev[device] = torch.from_numpy(self._packed).to(device)
        return self._dev[device]

    def __getstate__(self):
        st = dict(self.__dict__)
        st["_dev"] = {}
        return st

    def _check_fields(self, U, V, W, who):
        B = U.shape[0]
        su, sv = (B, self.Nx, self.Ny + 1, self.Nz), (B, self.Nx, self.Ny, self.Nz)
        if tuple(U.shape) != su or tuple(W.shape) != su or tuple(V.shape) != sv:
            raise RuntimeError(f"fnoengine {who}: expected U, W {su} and V {sv}, got {tuple(U.shape)}, {tuple(W.shape)}, "
                               f"{tuple(V.shape)}")
        for t, n in ((U, "U"), (V, "V"), (W, "W")):
            if not t.is_cuda:
                raise RuntimeError(f"fnoengine {who}: `{n}` must live on the GPU (got {t.device}); the engine has no CPU path")


def chanflow_rhs(grid, U, V, W, dPdx):
    """Fu, Fv, Fw = NSControlEnvMatlab.compute_rhs_py(U, V, W, dPdx) (libs/envs/control_env.py:429-530) for a batch of
    fields: U, W (B, Nx, Ny+1, Nz), V (B, Nx, Ny, Nz), fp32 or fp64; dPdx a float or a (B,) tensor.  Not differentiable
    (the reference uses it under autograd only through pde_loss -> chanflow_pde_loss)."""
    e = "chanflow_rhs"
    grid._check_fields(U, V, W, e)
    if U.dtype not in (torch.float32, torch.float64):
        raise RuntimeError(f"fnoengine {e}: U, V, W must share one dtype, float32 or float64")
    U, V, W = (_operand(e, n, t, U, dtype=U.dtype) for n, t in (("U", U), ("V", V), ("W", W)))
    B = U.shape[0]
    dp, dflt = None, 0.0
    if torch.is_tensor(dPdx) and (dPdx.numel() > 1 or (dPdx.is_cuda and B == 1)):      # a device value is read on the device
        dp = _operand(e, "dPdx", dPdx.to(device=U.device, dtype=U.dtype), U, dtype=U.dtype, numel=B).reshape(B)
    else:
        dflt = float(dPdx)
    Fu, Fv, Fw = torch.empty_like(U), torch.empty_like(V), torch.empty_like(W)
    g = grid.desc()
    m = _operand(e, "grid metrics", grid.metrics(U.device), U, dtype=torch.float64, numel=3 * (grid.Ny + 2))
    _call(e, U.device, "fno_chanflow_rhs", C.byref(g), B, 0 if U.dtype == torch.float32 else 1, m, U, V, W, dp, dflt, Fu, Fv, Fw,
          STREAM)
    return Fu, Fv, Fw


class _ChanflowPdeLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, grid, U, Vgt, V, W):
        e = "chanflow_pde_loss"
        B = U.shape[0]
        U, Vgt, V, W = (_operand(e, n, t, U) for n, t in (("U", U), ("Vgt", Vgt), ("V", V), ("W", W)))
        g = grid.desc()
        nws = _lib.lib().fno_chanflow_pde_loss_workspace_bytes(C.byref(g), B)
        ws = _bytes(nws, U.device)
        loss = torch.empty(1, dtype=torch.float32, device=U.device)
        m = _operand(e, "grid metrics", grid.metrics(U.device), U, dtype=torch.float64, numel=3 * (grid.Ny + 2))
        _call("chanflow_pde_loss_forward", U.device, "fno_chanflow_pde_loss_forward", C.byref(g), B, m, U, Vgt, V, W, loss, ws,
              nws, STREAM)
        ctx.save_for_backward(U, Vgt, V, W, ws, m)
        ctx.meta = (grid, B, nws)
        return loss[0]

    @staticmethod
    def backward(ctx, gl):
        U, Vgt, V, W, ws, m = ctx.saved_tensors
        grid, B, nws = ctx.meta
        g = grid.desc()
        dV = torch.empty_like(V)
        glc = _operand("chanflow_pde_loss backward", "gl", gl.contiguous().to(torch.float32), V, numel=1).reshape(1)
        _call("chanflow_pde_loss_backward", V.device, "fno_chanflow_pde_loss_backward", C.byref(g), B, m, U, Vgt, V, W, glc, dV,
              ws, nws, STREAM)
        return None, None, None, dV, None


def chanflow_pde_loss(grid, U, Vgt, V, W):
    """sum_b ||Fu(U,Vgt,W) - Fu(U,V,W)|| + ||Fv ..|| + ||Fw ..||: NSControlEnvMatlab.pde_loss (libs/envs/control_env.py:627-633)
    summed over the batch as the training loop does (run_pde_observers.py:226-230).  fp32 fields on the GPU;
    differentiable w.r.t. V (the predicted wall-normal velocity); the pressure gradient cancels and is not an argument."""
    grid._check_fields(U, V, W, "chanflow_pde_loss")
    if tuple(Vgt.shape) != tuple(V.shape):
        raise RuntimeError(f"fnoengine chanflow_pde_loss: Vgt {tuple(Vgt.shape)} must match V {tuple(V.shape)}")
    _require_cuda(U, "U")
    return _ChanflowPdeLossFn.apply(grid, U, Vgt, V, W)


# ----------------------------------------------------------------------------
# channel-flow environment step, float64 (libs/envs/control_env.py:533-613, 196-229, 186-303)
# ----------------------------------------------------------------------------
CHANFLOW_DIAG = ("sum_div", "mean_abs_U", "mean_abs_V", "mean_abs_W", "norm_U", "norm_V", "norm_W", "shear_stress", "bulk_velocity",
                 "p2_mean", "dpdx_finite_difference", "shear_stress_signed")      # columns of chanflow_diagnostics


class ChannelPoisson:
    """The Poisson table of a ChannelGrid (fno_chanflow_poisson_pack): twiddles, bulk-velocity weights and the Thomas
    factors of every wavenumber pair's wall-normal system.  Built once on the host, one device copy per GPU."""

    def __init__(self, grid):
        import numpy as np
        self.grid = grid
        g = grid.desc()
        self.nbytes = int(_lib.lib().fno_chanflow_poisson_table_bytes(C.byref(g)))
        if self.nbytes == 0:
            raise RuntimeError("fnoengine ChannelPoisson: " + _lib.lib().fno_last_error().decode("utf-8", "replace"))
        self.packed = np.zeros(self.nbytes // 8, dtype=np.float64)
        dp = C.POINTER(C.c_double)
        _lib.check(_lib.lib().fno_chanflow_poisson_pack(C.byref(g), grid.y.ctypes.data_as(dp), grid.ym.ctypes.data_as(dp),
                                                        grid.yg.ctypes.data_as(dp), self.packed.ctypes.data_as(dp), self.nbytes),
                   "chanflow_poisson_pack")
        self._dev = {}

    def table(self, device):
        if device not in self._dev:
            self._dev[device] = torch.from_numpy(self.packed).to(device)
        return self._dev[device]

    def __getstate__(self):
        st = dict(self.__dict__)
        st["_dev"] = {}
        return st


def chanflow_step_workspace(grid, B, device):
    """an uninitialised workspace for `B` environments (every step entry point takes one; a graph holds on to its own)"""
    g = grid.desc()
    n = _lib.lib().fno_chanflow_step_workspace_bytes(C.byref(g), B)
    if n == 0:
        raise RuntimeError("fnoengine chanflow step: " + _lib.lib().fno_last_error().decode("utf-8", "replace"))
    return _bytes(n, device)


def _chanflow_step_operands(e, grid, poisson, U, V, W, ws, layout):
    """checked state, metrics, table and workspace of a step entry point.  dtype code 1 = float64; any other dtype and a table
    built for another grid reach the engine as they are, which refuses both before it launches anything"""
    grid._check_fields(U, V, W, e)
    dt = U.dtype
    code = {torch.float64: 1, torch.float32: 0}.get(dt, -1)
    U, V, W = (_operand(e, n, t, U, dtype=dt, layout=layout) for n, t in (("U", U), ("V", V), ("W", W)))
    m = _operand(e, "grid metrics", grid.metrics(U.device), U, dtype=torch.float64, numel=3 * (grid.Ny + 2))
    tab = _operand(e, "Poisson table", poisson.table(U.device), U, dtype=torch.float64)
    B = U.shape[0]
    if ws is None:
        ws = chanflow_step_workspace(grid, B, U.device)
    ws = _operand(e, "workspace", ws, U, dtype=torch.uint8, layout="dense")
    return B, code, U, V, W, m, tab, ws


def chanflow_project(grid, poisson, U, V, W, ws=None):
    """The fractional-step projection (compute_projection_step, control_env.py:582-613) of a batch of float64 states,
    IN PLACE: divergence, Poisson solve per wavenumber pair, gradient correction of the interior rows, then the U, W ghost
    rows by reflection (V's wall rows are left as they are).  Returns U, V, W."""
    e = "chanflow_project"
    B, code, U, V, W, m, tab, ws = _chanflow_step_operands(e, grid, poisson, U, V, W, ws, "dense")
    g = grid.desc()
    _call(e, U.device, "fno_chanflow_project", C.byref(g), B, code, m, tab, tab.numel() * 8, U, V, W, ws, ws.numel(), STREAM)
    return U, V, W


def _per_sample(e, name, v, U):
    B = U.shape[0]
    if not torch.is_tensor(v):
        v = torch.full((B,), float(v), dtype=torch.float64, device=U.device)
    return _operand(e, name, v, U, dtype=torch.float64, numel=B, layout="dense")


def chanflow_wall_pressure(grid, poisson, U, V, W, dPdx, full=False, ws=None, out=None):
    """p1, p2 (B, Nx, Nz) of get_boundary_pressures (control_env.py:423-427): the Poisson solve on the divergence of the
    right-hand side (:196-229), observed at the two walls; with full=True also P (B, Nx, Ny-1, Nz).  dPdx: float or (B,)
    float64 tensor.  `out` = (p1, p2[, P]) to write into existing tensors."""
    e = "chanflow_wall_pressure"
    B, code, U, V, W, m, tab, ws = _chanflow_step_operands(e, grid, poisson, U, V, W, ws, "copy")
    dp = _per_sample(e, "dPdx", dPdx, U)
    shp = (B, grid.Nx, grid.Nz)
    if out is None:
        out = [torch.empty(shp, dtype=torch.float64, device=U.device) for _ in range(2)]
        if full:
            out.append(torch.empty((B, grid.Nx, grid.Ny - 1, grid.Nz), dtype=torch.float64, device=U.device))
    p1, p2 = (_operand(e, n, t, U, dtype=torch.float64, shape=shp, layout="dense") for n, t in zip(("p1", "p2"), out))
    P = _operand(e, "P", out[2], U, dtype=torch.float64, shape=(B, grid.Nx, grid.Ny - 1, grid.Nz), layout="dense") if full else None
    g = grid.desc()
    _call(e, U.device, "fno_chanflow_wall_pressure", C.byref(g), B, code, m, tab, tab.numel() * 8, U, V, W, dp, p1, p2, P, ws,
          ws.numel(), STREAM)
    return (p1, p2, P) if full else (p1, p2)


def chanflow_rk3_step(grid, poisson, U, V, W, opV1, opV2, dPdx, meanU0, dt, ws=None):
    """One boundary-controlled RK3 step (time_advance_RK3_py, control_env.py:533-580) of a batch of float64 states, IN PLACE
    on U, V, W and on dPdx, a (B,) float64 tensor; opV1, opV2 (B, Nx, Nz) are the wall-normal velocities imposed at the two
    walls, meanU0 (B,) the bulk velocity the pressure gradient holds.  Nothing is read back: the step never synchronises."""
    e = "chanflow_rk3_step"
    B, code, U, V, W, m, tab, ws = _chanflow_step_operands(e, grid, poisson, U, V, W, ws, "dense")
    shp = (B, grid.Nx, grid.Nz)
    v1, v2 = (_operand(e, n, t, U, dtype=torch.float64, shape=shp) for n, t in (("opV1", opV1), ("opV2", opV2)))
    if not torch.is_tensor(dPdx):
        raise _refuse(e, "dPdx", "be a (B,) float64 tensor (it is updated in place)", type(dPdx).__name__)
    dp, mu = _per_sample(e, "dPdx", dPdx, U), _per_sample(e, "meanU0", meanU0, U)
    g = grid.desc()
    _call(e, U.device, "fno_chanflow_rk3_step", C.byref(g), B, code, m, tab, tab.numel() * 8, U, V, W, v1, v2, dp, mu, float(dt), ws,
          ws.numel(), STREAM)
    return U, V, W, dp


def chanflow_diagnostics(grid, poisson, U, V, W, p2=None, out=None):
    """(B, 12) float64, columns CHANFLOW_DIAG: the scalars of the environment's `info` (control_env.py:186-303) in one launch;
    p2 (B, Nx, Nz) feeds the two pressure columns (0 without it)."""
    e = "chanflow_diagnostics"
    grid._check_fields(U, V, W, e)
    dt = U.dtype
    U, V, W = (_operand(e, n, t, U, dtype=dt) for n, t in (("U", U), ("V", V), ("W", W)))
    B = U.shape[0]
    m = _operand(e, "grid metrics", grid.metrics(U.device), U, dtype=torch.float64, numel=3 * (grid.Ny + 2))
    tab = _operand(e, "Poisson table", poisson.table(U.device), U, dtype=torch.float64)
    p2 = _operand(e, "p2", p2, U, dtype=torch.float64, shape=(B, grid.Nx, grid.Nz), optional=True)
    if out is None:
        out = torch.empty((B, len(CHANFLOW_DIAG)), dtype=torch.float64, device=U.device)
    out = _operand(e, "out", out, U, dtype=torch.float64, shape=(B, len(CHANFLOW_DIAG)), layout="dense")
    g = grid.desc()
    _call(e, U.device, "fno_chanflow_diagnostics", C.byref(g), B, {torch.float64: 1, torch.float32: 0}.get(dt, -1), m, tab,
          tab.numel() * 8, U, V, W, p2, out, STREAM)
    return out


class GraphedChannelStep:
    """chanflow_rk3_step + chanflow_wall_pressure of a fixed batch replayed as ONE graph.  The state, the controls, dPdx and
    the observations live in tensors the graph owns: write `opV1` / `opV2` (copy_), call step(), read `p1` / `p2`."""

    def __init__(self, grid, poisson, U, V, W, dPdx, meanU0, dt):
        self.grid, self.poisson, self.dt = grid, poisson, float(dt)
        self.U, self.V, self.W = (t.detach().clone().contiguous() for t in (U, V, W))
        B, dev = self.U.shape[0], self.U.device
        self.dPdx, self.meanU0 = _per_sample("GraphedChannelStep", "dPdx", dPdx, self.U).clone(), _per_sample("GraphedChannelStep", "meanU0", meanU0, self.U).clone()
        self.opV1 = torch.zeros((B, grid.Nx, grid.Nz), dtype=torch.float64, device=dev)
        self.opV2 = torch.zeros_like(self.opV1)
        self.p1, self.p2 = torch.zeros_like(self.opV1), torch.zeros_like(self.opV1)
        self.ws = chanflow_step_workspace(grid, B, dev)
        saved = [t.clone() for t in (self.U, self.V, self.W, self.dPdx)]
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):                      # one eager run loads the code objects before the capture
            self._body()
        torch.cuda.current_stream(dev).wait_stream(side)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self._body()
        for t, s in zip((self.U, self.V, self.W, self.dPdx), saved):
            t.copy_(s)

    def _body(self):
        chanflow_rk3_step(self.grid, self.poisson, self.U, self.V, self.W, self.opV1, self.opV2, self.dPdx, self.meanU0, self.dt,
                          ws=self.ws)
        chanflow_wall_pressure(self.grid, self.poisson, self.U, self.V, self.W, self.dPdx, ws=self.ws, out=(self.p1, self.p2))

    def step(self):
        self.graph.replay()
        return self.p1, self.p2


# ----------------------------------------------------------------------------
# closed-loop control (run_control.py): observation / action bridges, two-level diagnostics, running statistics
# ----------------------------------------------------------------------------
CONTROL_LOG = CHANFLOW_DIAG + ("dPdx",)      # columns of chanflow_diagnostics2: one row of a (T, B, 13) control log
STATS_MAX_FIELDS = _lib.FNO_CTRL_STATS_MAX


def _gpu_anchor(e, name, t):
    """the first operand of a float64 entry point (_require_cuda is the float32 one): a GPU tensor, or a refusal"""
    if not torch.is_tensor(t):
        raise _refuse(e, name, "be a tensor", type(t).__name__)
    if not t.is_cuda:
        raise _refuse(e, name, "live on the GPU (the engine has no CPU path)", t.device)
    return t


def _plane_stats(e, mean, std, anchor, plane):
    return (_operand(e, "mean", mean, anchor, dtype=torch.float64, numel=plane),
            _operand(e, "std", std, anchor, dtype=torch.float64, numel=plane))


def _strided_rows(e, name, t, anchor, B, plane, stride):
    """a dense float32 tensor read or written as B rows of `plane` floats, `stride` floats apart"""
    t = _operand(e, name, t, anchor, dtype=torch.float32, layout="dense")
    if stride < plane or t.numel() < (B - 1) * stride + plane:
        raise _refuse(e, name, f"hold {B} planes of {plane} floats {stride} apart", f"{t.numel()} elements, shape {tuple(t.shape)}")
    return t


def ctrl_encode(p, mean, std, eps=1e-5, out=None, batch_stride=None):
    """out[b * batch_stride + i] = float32((p[b].flatten()[i] - mean[i]) / (std[i] + eps)): NormalizerGivenMeanStd.encode on the
    float64 observation followed by .float() (run_control.py:139-141), in one launch.  p (B, Nx, Nz) float64; mean, std float64
    with Nx * Nz elements.  `out`: a dense float32 tensor, e.g. the persistent (B, 3, Nx, Nz) observer input with
    batch_stride = 3 * Nx * Nz (channel 0 is written, the grid channels are left alone); None: a new (B, Nx, Nz)."""
    e = "ctrl_encode"
    _gpu_anchor(e, "p", p)
    if p.dim() < 2:
        raise _refuse(e, "p", "be (B, Nx, Nz)", tuple(p.shape))
    B, plane = p.shape[0], p[0].numel()
    p = _operand(e, "p", p, p, dtype=torch.float64)
    mean, std = _plane_stats(e, mean, std, p, plane)
    if out is None:
        out, batch_stride = torch.empty(p.shape, dtype=torch.float32, device=p.device), plane
    stride = plane if batch_stride is None else int(batch_stride)
    out = _strided_rows(e, "out", out, p, B, plane, stride)
    _call(e, p.device, "fno_ctrl_encode", B, plane, p, mean, std, float(eps), out, stride, STREAM)
    return out


def ctrl_decode(y, mean, std, eps=1e-5, shape=None, batch_stride=None, scale=1.0, clip=0.0, zero_mean=False, out=None):
    """opV1, opV2 (B, Nx, Nz) float64 from the float32 model output: opV2 = y.double() * (std + eps) + mean
    (NormalizerGivenMeanStd.decode), then * scale, clamp to +-clip (0 = off) and, with zero_mean, minus each sample's own plane
    mean (run_control.py:223), in this order; opV1 = 0 (one-sided control, :154).  y: dense float32 holding B planes
    `batch_stride` floats apart (default: the plane); `shape` = (B, Nx, Nz) unless `out` = (opV1, opV2) gives it."""
    e = "ctrl_decode"
    _gpu_anchor(e, "y", y)
    if out is not None:
        shape = tuple(out[1].shape)
    if shape is None:
        raise _refuse(e, "shape", "be given as (B, Nx, Nz), or `out`", None)
    shape = tuple(int(v) for v in shape)
    B, plane = shape[0], math.prod(shape[1:])
    stride = plane if batch_stride is None else int(batch_stride)
    y = _strided_rows(e, "y", y, y, B, plane, stride)
    mean, std = _plane_stats(e, mean, std, y, plane)
    if out is None:
        out = (torch.empty(shape, dtype=torch.float64, device=y.device), torch.empty(shape, dtype=torch.float64, device=y.device))
    v1, v2 = (_operand(e, n, t, y, dtype=torch.float64, shape=shape, layout="dense") for n, t in zip(("opV1", "opV2"), out))
    _call(e, y.device, "fno_ctrl_decode", B, plane, y, stride, mean, std, float(eps), float(scale), float(clip), int(bool(zero_mean)),
          v1, v2, STREAM)
    return v1, v2


def chanflow_diagnostics2_workspace(grid, B, device):
    """the partial-sum workspace of chanflow_diagnostics2 for `B` environments on this grid (its size is checked exactly)"""
    g = grid.desc()
    n = _lib.lib().fno_chanflow_diagnostics2_workspace_bytes(C.byref(g), B)
    if n == 0:
        raise RuntimeError("fnoengine chanflow_diagnostics2: " + _lib.lib().fno_last_error().decode("utf-8", "replace"))
    return torch.empty(n, dtype=torch.uint8, device=device)


def chanflow_diagnostics2(grid, poisson, U, V, W, p2, dPdx, out=None, ws=None):
    """(B, 13) float64, columns CONTROL_LOG: chanflow_diagnostics and dPdx as a two-level reduction (a workgroup per wall-normal
    row and sample, then one per sample in a fixed order), written straight into `out`: a (B, 13) tensor or one row log[r] of a
    (T, B, 13) device log.  dPdx: the (B,) float64 device tensor of the step.  `ws`: chanflow_diagnostics2_workspace of this
    grid and batch."""
    e = "chanflow_diagnostics2"
    grid._check_fields(U, V, W, e)
    dt = U.dtype
    U, V, W = (_operand(e, n, t, U, dtype=dt) for n, t in (("U", U), ("V", V), ("W", W)))
    B, ncol = U.shape[0], len(CONTROL_LOG)
    m = _operand(e, "grid metrics", grid.metrics(U.device), U, dtype=torch.float64, numel=3 * (grid.Ny + 2))
    tab = _operand(e, "Poisson table", poisson.table(U.device), U, dtype=torch.float64)
    p2 = _operand(e, "p2", p2, U, dtype=torch.float64, shape=(B, grid.Nx, grid.Nz), optional=True)
    if not torch.is_tensor(dPdx):
        raise _refuse(e, "dPdx", "be a (B,) float64 tensor", type(dPdx).__name__)
    dp = _per_sample(e, "dPdx", dPdx, U)
    if out is None:
        out = torch.empty((B, ncol), dtype=torch.float64, device=U.device)
    out = _operand(e, "out", out, U, dtype=torch.float64, shape=(B, ncol), layout="keep")
    stride = out.stride(0) if B > 1 else ncol
    if out.stride(1) != 1 or stride < ncol:
        raise _refuse(e, "out", "have unit-stride rows at least 13 apart", f"strides {out.stride()}")
    g = grid.desc()
    need = _lib.lib().fno_chanflow_diagnostics2_workspace_bytes(C.byref(g), B)
    if ws is None:
        ws = chanflow_diagnostics2_workspace(grid, B, U.device)
    ws = _operand(e, "workspace", ws, U, dtype=torch.uint8, layout="dense")
    if ws.numel() != need:
        raise _refuse(e, "workspace", f"be the {need} bytes of this grid and a batch of {B}", f"{ws.numel()} bytes")
    _call(e, U.device, "fno_chanflow_diagnostics2", C.byref(g), B, {torch.float64: 1, torch.float32: 0}.get(dt, -1), m, tab,
          tab.numel() * 8, U, V, W, p2, dp, out, stride, ws, ws.numel(), STREAM)
    return out


def running_stats_update(fields, means, m2s, count):
    """One more snapshot into the running per-point statistics of up to eight fields, in ONE launch (the reference recomputes
    np.array(all_so_far).mean(0) / .std(0) on every collected step, run_control.py:245-293).  fields[k], means[k], m2s[k]:
    float64 tensors of one size per k, updated in place (Welford); `count`: snapshots including this one (1 initialises).
    std = sqrt(M2 / count), the population form like np.std."""
    e = "running_stats_update"
    fields, means, m2s = list(fields), list(means), list(m2s)
    if not 1 <= len(fields) <= STATS_MAX_FIELDS:
        raise _refuse(e, "fields", f"be 1..{STATS_MAX_FIELDS} tensors per launch", len(fields))
    if len(means) != len(fields) or len(m2s) != len(fields):
        raise _refuse(e, "means / m2s", f"have one tensor per field ({len(fields)})", (len(means), len(m2s)))
    if int(count) < 1:
        raise _refuse(e, "count", "be the number of snapshots including this one (>= 1)", count)
    anchor = _gpu_anchor(e, "fields[0]", fields[0])
    tab, keep = _lib.FnoCtrlStats(), []
    for k, (x, mu, m2) in enumerate(zip(fields, means, m2s)):
        x = _operand(e, f"fields[{k}]", x, anchor, dtype=torch.float64)
        mu = _operand(e, f"means[{k}]", mu, anchor, dtype=torch.float64, numel=x.numel(), layout="dense")
        m2 = _operand(e, f"m2s[{k}]", m2, anchor, dtype=torch.float64, numel=x.numel(), layout="dense")
        tab.x[k], tab.mean[k], tab.m2[k], tab.n[k] = _ptr(x), _ptr(mu), _ptr(m2), x.numel()
        keep.append(x)
    _call(e, anchor.device, "fno_ctrl_stats_update", C.byref(tab), len(fields), int(count), STREAM)


# ----------------------------------------------------------------------------
# optimal-observer policy (run_control.py:186-224): the objective and the Adam step on the wall action (k_action_opt.h)
# ----------------------------------------------------------------------------
ACTION_PARTS = ("loss", "field_norm", "action_norm")      # columns of ctrl_action_objective's `parts`


def _action_rows(e, name, t, anchor, B, plane):
    """a float32 tensor of B planes that the engine updates in place (the action, its two Adam moments)"""
    return _operand(e, name, t, anchor, dtype=torch.float32, numel=B * plane, layout="dense")


def ctrl_action_begin(opV2_0, mean, std, eps, a, x, batch_stride=None):
    """a[b] = float32(opV2_0[b]) and x[b * batch_stride + i] = float32((float64(a[b, i]) - mean[i]) / (std[i] + eps)): the leaf
    of the optimal-observer policy and its first observer input, in one launch.  opV2_0 (B, Nx, Nz) float64; a float32 with
    B * Nx * Nz elements and x the dense float32 observer input, both written in place."""
    e = "ctrl_action_begin"
    _gpu_anchor(e, "opV2_0", opV2_0)
    if opV2_0.dim() < 2:
        raise _refuse(e, "opV2_0", "be (B, Nx, Nz)", tuple(opV2_0.shape))
    B, plane = opV2_0.shape[0], opV2_0[0].numel()
    v0 = _operand(e, "opV2_0", opV2_0, opV2_0, dtype=torch.float64)
    mean, std = _plane_stats(e, mean, std, v0, plane)
    a = _action_rows(e, "a", a, v0, B, plane)
    stride = plane if batch_stride is None else int(batch_stride)
    x = _strided_rows(e, "x", x, v0, B, plane, stride)
    _call(e, v0.device, "fno_ctrl_action_begin", B, plane, v0, mean, std, float(eps), a, x, stride, STREAM)
    return a, x


def ctrl_action_workspace(B, planes, plane, device):
    """the partial-sum workspace of ctrl_action_objective for B environments, `planes` predicted planes of `plane` points"""
    n = _lib.lib().fno_ctrl_action_workspace_bytes(int(B), int(planes), int(plane))
    if n == 0:
        raise RuntimeError("fnoengine ctrl_action_objective: " + _lib.lib().fno_last_error().decode("utf-8", "replace"))
    return torch.empty(n, dtype=torch.uint8, device=device)


def ctrl_action_objective(y, a, mean, std, eps=1e-5, reg=0.1, parts=None, dy=None, ws=None):
    """The optimal-observer objective of every environment and its gradient with respect to the observer's output:
    field = float64(y) * (std + eps) + mean, parts[b] = (nf + reg * na, nf, na) with nf = |field[b]|_2 over all predicted
    planes and na = |float64(a[b])|_2 (columns ACTION_PARTS, float64), dy = float32(field / nf * (std + eps)), zero where
    nf == 0.  y (B, P, Nx, Nz[, 1]) float32, a (B, Nx * Nz) float32.  Fixed-order float64 sums in two launches: the same bits
    run to run and at every batch position.  `ws`: ctrl_action_workspace of this shape.  Returns (parts, dy)."""
    e = "ctrl_action_objective"
    _gpu_anchor(e, "y", y)
    if not torch.is_tensor(a) or a.dim() < 2 or y.dim() < 3 or a.shape[0] != y.shape[0]:
        raise _refuse(e, "a", "be (B, Nx * Nz) beside y (B, P, Nx, Nz)", getattr(a, "shape", type(a).__name__))
    B, plane = a.shape[0], a[0].numel()
    P = y.shape[1]
    y = _operand(e, "y", y, y, dtype=torch.float32, numel=B * P * plane)
    a = _operand(e, "a", a, y, dtype=torch.float32)
    mean, std = _plane_stats(e, mean, std, y, plane)
    if parts is None:
        parts = torch.empty((B, len(ACTION_PARTS)), dtype=torch.float64, device=y.device)
    parts = _operand(e, "parts", parts, y, dtype=torch.float64, shape=(B, len(ACTION_PARTS)), layout="dense")
    if dy is None:
        dy = torch.empty(y.shape, dtype=torch.float32, device=y.device)
    dy = _operand(e, "dy", dy, y, dtype=torch.float32, numel=y.numel(), layout="dense")
    need = _lib.lib().fno_ctrl_action_workspace_bytes(B, P, plane)
    if ws is None:
        ws = ctrl_action_workspace(B, P, plane, y.device)
    ws = _operand(e, "workspace", ws, y, dtype=torch.uint8, layout="dense")
    if ws.numel() != need:
        raise _refuse(e, "workspace", f"be the {need} bytes of a batch of {B} with {P} planes of {plane}", f"{ws.numel()} bytes")
    _call(e, y.device, "fno_ctrl_action_objective", B, P, plane, y, a, mean, std, float(eps), float(reg), parts, dy, ws, ws.numel(),
          STREAM)
    return parts, dy


def ctrl_action_update(dx, parts, mean, std, eps, a, exp_avg, exp_avg_sq, x, step, reg=0.1, lr=1e-3, betas=(0.9, 0.999),
                       adam_eps=1e-8, batch_stride=None):
    """One epoch's update of the optimal-observer action, in one launch and in place: g = float32(float64(dx) / (std + eps) +
    reg * float64(a) / na) with na = parts[:, 2] (the regulariser's term is zero where na == 0), torch.optim.Adam's float32 step
    number `step` on (a, g) (no weight decay, no amsgrad; step 1 initialises exp_avg / exp_avg_sq without reading them), and
    x = float32((float64(a) - mean) / (std + eps)), the observer input of the next epoch.  dx: the observer's input gradient
    (B, Nx * Nz) float32."""
    e = "ctrl_action_update"
    _gpu_anchor(e, "dx", dx)
    if not torch.is_tensor(parts) or parts.dim() != 2:
        raise _refuse(e, "parts", "be the (B, 3) float64 tensor of ctrl_action_objective", getattr(parts, "shape", type(parts).__name__))
    if int(step) < 1:
        raise _refuse(e, "step", "be the number of this Adam step (>= 1)", step)
    B = parts.shape[0]
    plane = dx.numel() // max(B, 1)
    dx = _operand(e, "dx", dx, dx, dtype=torch.float32, numel=B * plane)
    parts = _operand(e, "parts", parts, dx, dtype=torch.float64, shape=(B, len(ACTION_PARTS)))
    mean, std = _plane_stats(e, mean, std, dx, plane)
    a, m, v = (_action_rows(e, n, t, dx, B, plane) for n, t in (("a", a), ("exp_avg", exp_avg), ("exp_avg_sq", exp_avg_sq)))
    stride = plane if batch_stride is None else int(batch_stride)
    x = _strided_rows(e, "x", x, dx, B, plane, stride)
    _call(e, dx.device, "fno_ctrl_action_update", B, plane, dx, parts, mean, std, float(eps), float(reg), float(lr), float(betas[0]),
          float(betas[1]), float(adam_eps), int(step), a, m, v, x, stride, STREAM)
    return a


def ctrl_action_finish(a, out=None, shape=None):
    """opV2 (B, Nx, Nz) float64 = float64(a) minus each environment's own plane mean (run_control.py:223); the mean is a
    fixed-order sum inside one workgroup.  `shape` = (B, Nx, Nz) unless `out` gives it."""
    e = "ctrl_action_finish"
    _gpu_anchor(e, "a", a)
    if out is not None:
        shape = tuple(out.shape)
    if shape is None:
        shape = tuple(a.shape)
    shape = tuple(int(v) for v in shape)
    if len(shape) < 2:
        raise _refuse(e, "shape", "be (B, Nx, Nz)", shape)
    B, plane = shape[0], math.prod(shape[1:])
    a = _operand(e, "a", a, a, dtype=torch.float32, numel=B * plane)
    if out is None:
        out = torch.empty(shape, dtype=torch.float64, device=a.device)
    out = _operand(e, "opV2", out, a, dtype=torch.float64, shape=shape, layout="dense")
    _call(e, a.device, "fno_ctrl_action_finish", B, plane, a, out, STREAM)
    return out


# ----------------------------------------------------------------------------
# optimal-policy-observer policy (run_control.py:162-185): the glue between the policy network and the observer (k_policy_opt.h)
# ----------------------------------------------------------------------------
def _policy_rows(e, name, t, anchor, B, plane, dtype=torch.float32, layout="dense"):
    """a dense tensor of B planes of `plane` points, any shape"""
    return _operand(e, name, t, anchor, dtype=dtype, numel=B * plane, layout=layout)


def ctrl_policy_begin(opV2_0, p2, a0, pin):
    """a0 = float32(opV2_0) and pin = float32(p2) in one launch: the start action of the optimal-policy-observer policy and
    the policy network's input, the RAW wall pressure (run_control.py:163-166: no normaliser).  opV2_0, p2 (B, Nx, Nz)
    float64; a0, pin float32 with B * Nx * Nz elements, written in place."""
    e = "ctrl_policy_begin"
    _gpu_anchor(e, "opV2_0", opV2_0)
    if opV2_0.dim() < 2:
        raise _refuse(e, "opV2_0", "be (B, Nx, Nz)", tuple(opV2_0.shape))
    B, plane = opV2_0.shape[0], opV2_0[0].numel()
    v0 = _operand(e, "opV2_0", opV2_0, opV2_0, dtype=torch.float64)
    p2 = _policy_rows(e, "p2", p2, v0, B, plane, dtype=torch.float64, layout="copy")
    a0, pin = _policy_rows(e, "a0", a0, v0, B, plane), _policy_rows(e, "pin", pin, v0, B, plane)
    _call(e, v0.device, "fno_ctrl_policy_begin", B, plane, v0, p2, a0, pin, STREAM)
    return a0, pin


def ctrl_policy_compose(a0, res, x, opV2):
    """x = a0 + res (one float32 add) and opV2 = float64(x) in the same pass: the observer's input and the action the loop
    applies (run_control.py:170, 185).  a0 (B, Nx * Nz) float32; res, x float32 and opV2 float64 with the same number of
    elements; x and opV2 are written in place."""
    e = "ctrl_policy_compose"
    _gpu_anchor(e, "a0", a0)
    if a0.dim() < 2:
        raise _refuse(e, "a0", "be (B, Nx * Nz)", tuple(a0.shape))
    B, plane = a0.shape[0], a0[0].numel()
    a0 = _operand(e, "a0", a0, a0, dtype=torch.float32)
    res = _policy_rows(e, "res", res, a0, B, plane, layout="copy")
    x = _policy_rows(e, "x", x, a0, B, plane)
    opV2 = _policy_rows(e, "opV2", opV2, a0, B, plane, dtype=torch.float64)
    _call(e, a0.device, "fno_ctrl_policy_compose", B, plane, a0, res, x, opV2, STREAM)
    return x, opV2


def ctrl_policy_unit_stats(plane, device):
    """(mean, std) = (zeros, ones), float64 with `plane` points: the statistics ctrl_policy_objective hands the objective"""
    return (torch.zeros(int(plane), dtype=torch.float64, device=device), torch.ones(int(plane), dtype=torch.float64, device=device))


def ctrl_policy_objective(y, x, reg=0.1, parts=None, dy=None, ws=None, unit=None):
    """The optimal-policy-observer objective |y[b]|_2 + reg * |x[b]|_2 of every environment and dy = float32(float64(y) / nf):
    ctrl_action_objective as it stands (its kernels, reduction order, workspace and ACTION_PARTS columns), called with
    a := x and unit statistics mean = 0, std = 1, eps = 0.  The reference feeds the observer the raw action and reads raw
    planes (run_control.py:171-173: no encode, no decode), and unit statistics are exactly that: S = 1.0 + 0.0 = 1.0, the
    product float64(y) * 1.0 and the sum + 0.0 return float64(y) itself (a negative zero becomes a positive one, whose
    square and whose quotient by nf > 0 round to the same float32 magnitude 0), and dy = field / nf * 1.0 is the quotient
    rounded once; no operation of the kernel rounds anything it would not round without the statistics.  y (B, P, Nx, Nz[, 1])
    float32, x float32 with B * Nx * Nz elements; `unit`: ctrl_policy_unit_stats of this plane (made here when absent - pass
    it inside a graph capture).  Returns (parts, dy)."""
    e = "ctrl_policy_objective"
    _gpu_anchor(e, "y", y)
    if not torch.is_tensor(x) or y.dim() < 3 or x.dim() < 1 or x.shape[0] != y.shape[0]:
        raise _refuse(e, "x", "hold B planes beside y (B, P, Nx, Nz)", getattr(x, "shape", type(x).__name__))
    B = y.shape[0]
    plane = x.numel() // max(B, 1)
    if unit is None:
        unit = ctrl_policy_unit_stats(plane, y.device)
    return ctrl_action_objective(y, x.reshape(B, plane), unit[0], unit[1], 0.0, reg=reg, parts=parts, dy=dy, ws=ws)


def ctrl_policy_grad(dx, x, parts, reg=0.1, out=None):
    """g = float32(float64(dx) + reg * float64(x) / na) with na = parts[:, 2] (g = dx where na == 0): the gradient of
    |y|_2 + reg * |x|_2 with respect to the policy's output res (x = a0 + res), assembled in float64 and rounded once.  dx:
    the observer's input gradient given ctrl_policy_objective's dy; dx, x float32 with B * Nx * Nz elements; parts (B, 3)."""
    e = "ctrl_policy_grad"
    _gpu_anchor(e, "dx", dx)
    if not torch.is_tensor(parts) or parts.dim() != 2:
        raise _refuse(e, "parts", "be the (B, 3) float64 tensor of ctrl_policy_objective", getattr(parts, "shape", type(parts).__name__))
    B = parts.shape[0]
    plane = dx.numel() // max(B, 1)
    dx = _policy_rows(e, "dx", dx, dx, B, plane, layout="copy")
    x = _policy_rows(e, "x", x, dx, B, plane, layout="copy")
    parts = _operand(e, "parts", parts, dx, dtype=torch.float64, shape=(B, len(ACTION_PARTS)))
    if out is None:
        out = torch.empty(dx.shape, dtype=torch.float32, device=dx.device)
    out = _policy_rows(e, "g", out, dx, B, plane)
    _call(e, dx.device, "fno_ctrl_policy_grad", B, plane, dx, x, parts, float(reg), out, STREAM)
    return out


# ----------------------------------------------------------------------------
# NSControlEnv2D: the 2-D periodic channel (libs/envs/ns_control_2d.py), float64, one workgroup per environment
# ----------------------------------------------------------------------------
NS2D_SOLVE_OUT = ("bulk_v", "steps", "status")
NS2D_STATUS = ("converged", "max_step", "cap")
NS2D_FIXED_OUT = ("result_f", "flow", "error", "bisections", "steps", "status")
NS2D_FIXED_STATUS = ("ok", "overflow", "cap")
NS2D_DIAG = ("drag_reduction/1_shear_stress", "drag_reduction/2_1_mass_flow", "drag_reduction/2_2_v_velocity",
             "drag_reduction/3_1_pressure_mean", "drag_reduction/3_2_dPdx_required", "drag_reduction/4_1_-|divergence|",
             "drag_reduction/4_2_speed_norm")


class Ns2dGrid(typing.NamedTuple):
    """(ny, nx) points, periodic in x with all nx columns distinct, walls at rows 0 and ny-1; nit Jacobi sweeps per step"""
    nx: int
    ny: int
    nit: int
    dx: float
    dy: float
    dt: float
    rho: float

    def desc(self):
        return _lib.FnoNs2dGrid(int(self.nx), int(self.ny), int(self.nit), float(self.dx), float(self.dy), float(self.dt),
                                float(self.rho))


def _ns2d_operands(e, grid, p, u, v, nu, bc_lo, bc_hi, layout):
    """checked state, viscosity and wall rows of an ns2d entry point; the grid's extents reach the engine as they are, which
    refuses what it does not support before it launches anything"""
    _gpu_anchor(e, "p", p)
    if p.dim() != 3 or tuple(p.shape[1:]) != (grid.ny, grid.nx):
        raise _refuse(e, "p", f"be (B, {grid.ny}, {grid.nx}), the grid's (B, ny, nx)", tuple(p.shape))
    B = p.shape[0]
    p, u, v = (_operand(e, n, t, p, dtype=torch.float64, shape=p.shape, layout=layout) for n, t in (("p", p), ("u", u), ("v", v)))
    nu = _per_sample(e, "nu", nu, p)
    lo, hi = (_operand(e, n, t, p, dtype=torch.float64, shape=(B, grid.nx), optional=True) for n, t in (("bc_lo", bc_lo), ("bc_hi", bc_hi)))
    return B, p, u, v, nu, lo, hi


def ns2d_solve(grid, p, u, v, F, nu, bc_lo=None, bc_hi=None, max_step=-1, u_diff_thre=1e-2, step_cap=5000, update_state=True,
               un=None, vn=None, out=None):
    """NSControlEnv2D.solve (ns_control_2d.py:359-491) of a batch of float64 states (B, ny, nx) in one launch: F, nu floats or
    (B,) tensors, bc_lo / bc_hi (B, nx) wall-normal velocities at rows 0 / ny-1 (None: zero).  Steps while
    udiff > u_diff_thre; max_step > 1 caps (so 1 and -1 run to convergence, as the reference), more than step_cap steps end
    the launch.  update_state: p, u, v are advanced IN PLACE (and un, vn written when given) unless the cap was hit.
    Returns (B, 3) float64, columns NS2D_SOLVE_OUT; status indexes NS2D_STATUS.  Nothing is read back here."""
    e = "ns2d_solve"
    B, p, u, v, nu, lo, hi = _ns2d_operands(e, grid, p, u, v, nu, bc_lo, bc_hi, "dense" if update_state else "copy")
    F = _per_sample(e, "F", F, p)
    un, vn = (_operand(e, n, t, p, dtype=torch.float64, shape=p.shape, optional=True, layout="dense") for n, t in (("un", un), ("vn", vn)))
    if out is None:
        out = torch.empty((B, len(NS2D_SOLVE_OUT)), dtype=torch.float64, device=p.device)
    out = _operand(e, "out", out, p, dtype=torch.float64, shape=(B, len(NS2D_SOLVE_OUT)), layout="dense")
    g = grid.desc()
    _call(e, p.device, "fno_ns2d_solve", C.byref(g), B, p, u, v, un, vn, F, nu, lo, hi, int(max_step), float(u_diff_thre),
          int(step_cap), int(bool(update_state)), out, STREAM)
    return out


def ns2d_fixed_mass(grid, p, u, v, F, nu, target, min_f, max_f, bc_lo=None, bc_hi=None, u_diff_thre=1e-2, step_cap=5000,
                    max_bisect=500, error_threshold=1e-4, out=None):
    """NSControlEnv2D.solve_fixed_mass (:493-536) in one launch: converged solves at min_f and max_f from the given state, then
    bisection on the force towards the bulk velocity `target`; F is what a target outside the bracket returns.  Every
    per-environment scalar is a float or a (B,) tensor.  The state is read only.  Returns (B, 6) float64, columns
    NS2D_FIXED_OUT; status indexes NS2D_FIXED_STATUS."""
    e = "ns2d_fixed_mass"
    B, p, u, v, nu, lo, hi = _ns2d_operands(e, grid, p, u, v, nu, bc_lo, bc_hi, "copy")
    F, target, min_f, max_f = (_per_sample(e, n, t, p) for n, t in (("F", F), ("target", target), ("min_f", min_f), ("max_f", max_f)))
    if out is None:
        out = torch.empty((B, len(NS2D_FIXED_OUT)), dtype=torch.float64, device=p.device)
    out = _operand(e, "out", out, p, dtype=torch.float64, shape=(B, len(NS2D_FIXED_OUT)), layout="dense")
    g = grid.desc()
    _call(e, p.device, "fno_ns2d_fixed_mass", C.byref(g), B, p, u, v, F, nu, target, min_f, max_f, lo, hi, float(u_diff_thre),
          int(step_cap), int(max_bisect), float(error_threshold), out, STREAM)
    return out


def ns2d_diagnostics(grid, p, u, v, nu, dpdx=None, out=None, ptop=None):
    """The seven drag_reduction scalars of NSControlEnv2D.step (:562-581) as (B, 7) float64, columns NS2D_DIAG, and the top-wall
    pressure row p[:, -1, :] as (B, nx); dpdx: (B,) tensor or float for drag_reduction/3_2_dPdx_required (None: -1)."""
    e = "ns2d_diagnostics"
    B, p, u, v, nu, _, _ = _ns2d_operands(e, grid, p, u, v, nu, None, None, "copy")
    dpdx = None if dpdx is None else _per_sample(e, "dpdx", dpdx, p)
    if out is None:
        out = torch.empty((B, len(NS2D_DIAG)), dtype=torch.float64, device=p.device)
    out = _operand(e, "out", out, p, dtype=torch.float64, shape=(B, len(NS2D_DIAG)), layout="dense")
    if ptop is None:
        ptop = torch.empty((B, grid.nx), dtype=torch.float64, device=p.device)
    ptop = _operand(e, "ptop", ptop, p, dtype=torch.float64, shape=(B, grid.nx), layout="dense")
    g = grid.desc()
    _call(e, p.device, "fno_ns2d_diagnostics", C.byref(g), B, p, u, v, nu, dpdx, out, ptop, STREAM)
    return out, ptop


class GraphedControlLoop:
    """One control iteration (action from the observation, RK3 step, wall pressure, diagnostics) replayed as ONE graph, captured
    on one stream with no forked branches, like GraphedChannelStep.  `body`: a callable that runs the iteration on persistent
    tensors; `state`: the tensors it updates in place, restored after the eager run that loads the code objects."""

    def __init__(self, body, state, device):
        saved = [t.clone() for t in state]
        side = torch.cuda.Stream(device=device)
        side.wait_stream(torch.cuda.current_stream(device))
        with torch.cuda.stream(side):
            body()
        torch.cuda.current_stream(device).wait_stream(side)
        for t, s in zip(state, saved):
            t.copy_(s)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            body()
        for t, s in zip(state, saved):
            t.copy_(s)

    def replay(self):
        self.graph.replay()


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


# ----------------------------------------------------------------------------
# device-resident training data: a batch gathered, normalised and cast from a pool of raw snapshots in one launch
# ----------------------------------------------------------------------------
_DATA_DTYPES = {torch.float32: 0, torch.float64: 1}      # the header's dtype codes (fno_chanflow_rhs)


def _data_indices(e, idx, n_src):
    """the host check of a gather's indices: a CPU int64 vector inside [0, n_src); returns how many there are"""
    if not torch.is_tensor(idx) or idx.is_cuda or idx.dtype != torch.int64 or idx.dim() != 1:
        raise _refuse(e, "idx", "be a CPU int64 vector (it is checked on the host)",
                      f"{idx.device}, {idx.dtype}, shape {tuple(idx.shape)}" if torch.is_tensor(idx) else type(idx).__name__)
    if idx.numel() and not (0 <= int(idx.min()) and int(idx.max()) < n_src):
        raise _refuse(e, "idx", f"lie in [0, {n_src})", f"min {int(idx.min())}, max {int(idx.max())}")
    return idx.numel()


def data_gather(pool, idx, view, mean=None, std=None, eps=1e-5, out=None, out_stride=None):
    """out[e].flatten()[i * cols + j] = float32(f(pool[idx[e]].flatten()[offset + i * row_stride + j * col_stride])) for the view
    (offset, row_stride, col_stride, rows, cols): f = (x - mean[i, j]) / (std[i, j] + eps) in the type the host expression
    promotes to (NormalizerGivenMeanStd.encode, then .float()), or the identity when mean and std are None.  pool: a dense
    float32 / float64 GPU tensor (n_src, ...); idx: a CPU int64 vector, checked against 0 <= idx < n_src here, before anything is
    launched, and uploaded afterwards; mean, std: GPU tensors of one dtype with rows * cols elements.  `out`: a dense float32
    tensor written as len(idx) planes `out_stride` floats apart from its first element (e.g. `target.view(-1)[p * X * Z:]` with
    out_stride = P * X * Z fills plane p of a (B, T, P, X, Z) target and leaves the others alone); None: a new
    (len(idx), rows, cols).  One launch (k_data_gather)."""
    e = "data_gather"
    _gpu_anchor(e, "pool", pool)
    if pool.dtype not in _DATA_DTYPES:
        raise _refuse(e, "pool", "be float32 or float64", pool.dtype)
    if pool.dim() < 1 or pool.numel() == 0:
        raise _refuse(e, "pool", "be (n_src, ...) with at least one element", tuple(pool.shape))
    pool = _operand(e, "pool", pool, pool, dtype=pool.dtype, layout="dense")
    n_src, snap = pool.shape[0], pool[0].numel()
    count = _data_indices(e, idx, n_src)
    offset, row_stride, col_stride, rows, cols = (int(v) for v in view)
    if rows < 1 or cols < 1 or min(offset, row_stride, col_stride) < 0 or \
            offset + (rows - 1) * row_stride + (cols - 1) * col_stride >= snap:
        raise _refuse(e, "view", f"be (offset, row_stride, col_stride, rows, cols) inside a snapshot of {snap} elements", tuple(view))
    plane = rows * cols
    if (mean is None) != (std is None):
        raise _refuse(e, "mean / std", "be given together or not at all", "one of them")
    stat = 0
    if mean is not None:
        if not torch.is_tensor(mean) or mean.dtype not in _DATA_DTYPES:
            raise _refuse(e, "mean", "be a float32 or float64 tensor", getattr(mean, "dtype", type(mean).__name__))
        stat = _DATA_DTYPES[mean.dtype]
        mean = _operand(e, "mean", mean, pool, dtype=mean.dtype, numel=plane)
        std = _operand(e, "std", std, pool, dtype=mean.dtype, numel=plane)
    if out is None:
        out, out_stride = torch.empty((count, rows, cols), dtype=torch.float32, device=pool.device), plane
    stride = plane if out_stride is None else int(out_stride)
    out = _operand(e, "out", out, pool, dtype=torch.float32, layout="dense")
    if stride < plane or (count and out.numel() < (count - 1) * stride + plane):
        raise _refuse(e, "out", f"hold {count} planes of {plane} floats {stride} apart", f"{out.numel()} elements, shape {tuple(out.shape)}")
    if count == 0:
        return out
    idx_dev = idx.to(pool.device)        # (never through torch.empty / _bytes: an index buffer is not poisoned, tests/hygiene.py)
    _call(e, pool.device, "fno_data_gather", _DATA_DTYPES[pool.dtype], stat, pool, n_src, snap, offset, row_stride, col_stride,
          rows, cols, idx_dev, count, mean, std, float(eps), out, stride, STREAM)
    return out


# ----------------------------------------------------------------------------
# device-resident PINO training data: a batch (u, a_in) of a MultipleReynoldsKFaDataset from its resident tensors
# ----------------------------------------------------------------------------
def _data_out(e, out, anchor, shape, align=4):
    """a gather's output: new, or the caller's dense float32 buffer of exactly that many elements (e.g. a static input of a
    captured step) whose first element is aligned to `align` bytes; returned in `shape`"""
    if out is None:
        return torch.empty(shape, dtype=torch.float32, device=anchor.device)
    if not torch.is_tensor(out):
        raise _refuse(e, "out", "be a tensor", type(out).__name__)
    out = _operand(e, "out", out, anchor, dtype=torch.float32, numel=math.prod(shape), layout="dense")
    if out.data_ptr() % align:
        raise _refuse(e, "out", f"start on a {align}-byte boundary", f"address {out.data_ptr():#x}")
    return out.view(shape)


def data_transpose_gather(pool, idx, out=None):
    """out[e] = pool[idx[e]].transpose(0, 1) as words: pool (n_src, rows, cols) dense float32 on the GPU -> (len(idx), cols, rows),
    every bit pattern unchanged.  idx: a CPU int64 vector, checked against 0 <= idx < n_src here, before anything is launched, and
    uploaded afterwards.  `out`: a dense float32 tensor of len(idx) * rows * cols elements that is written in place (any 4-byte
    alignment) and returned in the result's shape; None: a new tensor.  One launch (k_data_transpose_gather)."""
    e = "data_transpose_gather"
    _gpu_anchor(e, "pool", pool)
    if pool.dim() != 3 or pool.numel() == 0:
        raise _refuse(e, "pool", "be (n_src, rows, cols) with at least one element", tuple(pool.shape))
    pool = _operand(e, "pool", pool, pool, layout="dense")
    n_src, rows, cols = pool.shape
    count = _data_indices(e, idx, n_src)
    out = _data_out(e, out, pool, (count, cols, rows))
    if count == 0:
        return out
    idx_dev = idx.to(pool.device)        # (never through torch.empty / _bytes: an index buffer is not poisoned, tests/hygiene.py)
    _call(e, pool.device, "fno_data_transpose_gather", pool, n_src, rows, cols, idx_dev, count, out, rows * cols, STREAM)
    return out


def pino_input(a0, idx, gx, gy, gt, out=None):
    """out[e, x, y, k] = (gx[x], gy[y], gt[k], a0[idx[e], x, y]): the (x, y, t, u0) input of the PINO observers, channels-last
    (len(idx), s1, s2, t, 4), from a0 (n_src, s1, s2) and the axis vectors gx (s1), gy (s2), gt (t) - dense float32 on the GPU,
    moved as words.  idx: a CPU int64 vector, checked against 0 <= idx < n_src here, before anything is launched, and uploaded
    afterwards.  `out`: a dense float32 tensor of that many elements on a 16-byte boundary, written in place and returned in the
    result's shape; None: a new tensor.  One launch (k_pino_input)."""
    e = "pino_input"
    _gpu_anchor(e, "a0", a0)
    if a0.dim() != 3 or a0.numel() == 0:
        raise _refuse(e, "a0", "be (n_src, s1, s2) with at least one element", tuple(a0.shape))
    a0 = _operand(e, "a0", a0, a0, layout="dense")
    n_src, s1, s2 = a0.shape
    axes = []
    for name, g, n in (("gx", gx, s1), ("gy", gy, s2), ("gt", gt, None)):
        if not torch.is_tensor(g) or g.dim() != 1 or g.numel() == 0:
            raise _refuse(e, name, "be a vector with at least one element", tuple(g.shape) if torch.is_tensor(g) else type(g).__name__)
        axes.append(_operand(e, name, g, a0, numel=n))
    t = axes[2].numel()
    count = _data_indices(e, idx, n_src)
    out = _data_out(e, out, a0, (count, s1, s2, t, 4), align=16)
    if count == 0:
        return out
    idx_dev = idx.to(a0.device)          # (as above)
    _call(e, a0.device, "fno_pino_input", a0, n_src, idx_dev, count, *axes, s1, s2, t, out, STREAM)
    return out
