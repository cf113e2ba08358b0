"""The fused Fourier stacks: the whole FNO model, block stacks, the RNO block tail and the fan-out.  Home of _model_plans.
"""
import ctypes as C

import torch

from .. import _lib
from ._core import (
    _bytes, _call, default_gelu_mask, _operand, _plan_available, plane_size, _ptr, _ptr_array, _require_cuda, row_tiling,
    STREAM)
from .spectral import (
    _Cfg, _check_corner_weights, _direct_views, _fill_params, _fresh_grads, _notify_direct, _real_views, _saved_params)

_model_plans = {}


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
