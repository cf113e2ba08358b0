"""Fused Adam: the step, the run-compacted step and the replay of dead slices.
"""
import ctypes as C

import torch

from .. import _lib
from ._core import _call, _operand, _require_cuda, STREAM


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
