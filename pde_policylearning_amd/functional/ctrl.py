"""Closed-loop control on the channel-flow solver: observation / action bridges, running statistics, the action and policy
optimisers, the captured control loop.
"""
import ctypes as C
import math

import torch

from .. import _lib
from ._core import _call, _gpu_anchor, _operand, _ptr, _refuse, STREAM

# ----------------------------------------------------------------------------
# closed-loop control (run_control.py): observation / action bridges, running statistics
# ----------------------------------------------------------------------------
STATS_MAX_FIELDS = _lib.FNO_CTRL_STATS_MAX


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
