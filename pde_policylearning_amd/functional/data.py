"""Device-resident training data: batches gathered, transposed and assembled by engine kernels.
"""
import math

import torch

from ._core import _call, _gpu_anchor, _operand, _refuse, STREAM


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
