"""What every family of engine wrappers shares: the operand check, the call, the shape rules.

The C ABI takes raw pointers and cannot see a tensor's device, dtype or extent, so the wrappers are where they are checked.
Two helpers carry that ("The Python bridge"):
  _operand   every tensor passes through it before its address is taken: same device as the entry point's anchor (its first
             operand, itself through _require_cuda), the expected dtype, the stated extent; returns it contiguous.
  _call      every launching engine function is called through it: enters the anchor's device, reads the current stream
             there, turns tensors into addresses, calls, and raises on a non-zero return code.
Every forward / backward of the sibling modules reads: check operands, allocate, call.  This module imports none of them.
"""
import ctypes as C
import math

import torch

from .. import _lib

_Tensor = torch.Tensor


def _require_cuda(t, name):
    if not t.is_cuda:
        raise RuntimeError(f"fnoengine: `{name}` must live on the GPU (got {t.device}); "
                           "the engine has no CPU path")
    if t.dtype != torch.float32:
        raise RuntimeError(f"fnoengine: `{name}` must be float32 (got {t.dtype})")


def _gpu_anchor(e, name, t):
    """the first operand of a float64 entry point (_require_cuda is the float32 one): a GPU tensor, or a refusal"""
    if not torch.is_tensor(t):
        raise _refuse(e, name, "be a tensor", type(t).__name__)
    if not t.is_cuda:
        raise _refuse(e, name, "live on the GPU (the engine has no CPU path)", t.device)
    return t


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


def _per_sample(e, name, v, U):
    B = U.shape[0]
    if not torch.is_tensor(v):
        v = torch.full((B,), float(v), dtype=torch.float64, device=U.device)
    return _operand(e, name, v, U, dtype=torch.float64, numel=B, layout="dense")


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
