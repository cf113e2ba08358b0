"""What the Sobolev / L2 training losses (csrc/k_sobolev_loss.h, functional.sobolev_loss, neuralop.training.losses LpLoss and
H1Loss) are held to: a helper module, not a conftest.

`restated` states LpLoss (p = 2) and H1Loss of the reference (neuralop/training/losses.py:62-277) with the EXPLICIT adjoint in
one dtype; in float64 it is the truth, in float32 the yardstick.  tests/golden/sobolev_loss_small.npz holds the reference's
own float32 values and gradients and ties the restatement to it (tests/test_sobolev_loss_host.py).

    x, y (*lead, n_1 .. n_d), h_k = L_k / n_k, e = x - y
    D_k v[i] = (v[i+1] - v[i-1]) / (2 h_k) mod n_k;  fixed axis: D_k v[0] = (v[1] - v[0]) / h_k, D_k v[n-1] = (v[n-1] - v[n-2]) / h_k
    D_k^T r  = (r[i-1] - r[i+1]) / (2 h_k) mod n_k;  fixed axis: the same with r[0], r[n-1] zeroed first, then
               -r[0]/h at 0, +r[0]/h at 1, +r[n-1]/h at n-1, -r[n-1]/h at n-2
    num = sum e^2 [+ sum_k sum (D_k e)^2],  den = the same of y  (order 0: LpLoss, order 1: H1Loss), per plane
    rel = sqrt(num / den),  abs = sqrt(prod(h) num);  then sum / mean over reduce_dims with keepdim, then squeeze
    dx = g_plane / sqrt(num den) (e + sum_k D_k^T D_k e)   or   g_plane sqrt(prod h) / sqrt(num) (...);  0 where num == 0

Input families, built in float64 from oracle.detfill and rounded once:
  white   x, y uniform +-1
  smooth  three low sine modes per field plus 5 % noise
  near    x = y (1 + 1e-3 fill)
  offset  y = 100 + fill, x = 100 + fill

Criterion: tests.judging.judge_budget (slack BUDGET_SLACK), floor FLOOR_GATE = 2e-6; a float32 yardstick at or above CAP = 0.1
is a failure by itself, so no row is ever left out.  Every figure goes to profiles/r23_sobolev_loss_errors.txt before anything
is asserted."""
import functools
import math
import os

import numpy as np
import torch

from oracle.detfill import name_seed, unit_fill
from tests.burgers_cases import scalar_err  # noqa: F401
from tests.judging import SectionLog, rel_err
from tests.step_tail_cases import FLOOR_GATE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
LOG = SectionLog(os.path.join(ROOT, "profiles", "r23_sobolev_loss_errors.txt"))
FLOOR = FLOOR_GATE
CAP = 0.1
# csrc/k_sobolev_loss.h: cells per workgroup of the flattened plane at order 0, and the tiles of d = 1, 2, 3
T0, T1, T2, T3 = 2048, 1024, (16, 64), (4, 8, 64)
FAMILIES = ("white", "smooth", "near", "offset")
# (shape, d).  1-D: extents 2, 3, 5; one tile, one cell into the second, one into the third; 1024; more than 64 tiles a plane.
# 2-D: extents 2 .. 5; odd; the workload's 61 and 64; one cell past the tile on each axis.  3-D likewise.
SHAPES = tuple(dict.fromkeys([
    ((2, 3, 2), 1), ((2, 2, 3), 1), ((2, 2, 5), 1), ((2, 1, T1), 1), ((2, 1, T1 + 1), 1), ((2, 1, 2 * T1 + 1), 1),
    ((2, 1, 1024), 1), ((1, 1, 65 * T1 + 3), 1),
    ((2, 2, 2, 3), 2), ((2, 2, 5, 4), 2), ((3, 2, 17, 33), 2), ((2, 3, 61, 61), 2), ((2, 1, 64, 64), 2),
    ((2, 1, T2[0] + 1, T2[1] + 1), 2),
    ((2, 1, 2, 3, 4), 3), ((2, 2, 5, 6, 7), 3), ((1, 1, 16, 16, 16), 3), ((1, 1, T3[0] + 1, T3[1] + 1, T3[2] + 1), 3)]))
GOLDEN_SHAPES = (((2, 3, 5), 1), ((3, 2, 5, 6), 2), ((2, 1, 4, 5, 3), 3))
L_DEFAULT = 2 * math.pi


def shape_id(shape, d):
    return f"d{d}_" + "x".join(str(n) for n in shape)


def fix_modes(d):
    """periodic, all fixed, and for d >= 2 the mixed per-axis flags"""
    modes = [(False,) * d, (True,) * d]
    if d == 2:
        modes += [(True, False), (False, True)]
    if d == 3:
        modes += [(True, False, True), (False, True, False)]
    return modes


def uniform_h(shape, d, L=L_DEFAULT):
    L = [L] * d if isinstance(L, float) else list(L)
    return [L[-j] / shape[-j] for j in range(d, 0, -1)]


@functools.lru_cache(maxsize=None)
def make_inputs(family, shape, d):
    """(x, y) float32 on the CPU"""
    tag = f"sobolev.{family}.{shape_id(shape, d)}"
    fill = lambda name: unit_fill(shape, name_seed(f"{tag}.{name}"))      # noqa: E731

    def smooth(name):
        lead = shape[:len(shape) - d]
        v = np.zeros(shape)
        for m in range(1, 4):
            term = unit_fill(lead, name_seed(f"{tag}.{name}.c{m}")).reshape(lead + (1,) * d)
            for k in range(d):
                n = shape[len(lead) + k]
                ph = math.pi * unit_fill(lead, name_seed(f"{tag}.{name}.p{m}.{k}")).reshape(lead + (1,) * d)
                grid = (2 * math.pi * m * np.arange(n) / n).reshape((1,) * (len(lead) + k) + (n,) + (1,) * (d - 1 - k))
                term = term * np.sin(grid + ph)
            v = v + term
        return v + 0.05 * fill(name + ".noise")
    if family == "white":
        x, y = fill("x"), fill("y")
    elif family == "smooth":
        x, y = smooth("x"), smooth("y")
    elif family == "near":
        y = fill("y")
        x = y * (1.0 + 1e-3 * fill("x"))
    elif family == "offset":
        x, y = 100.0 + fill("x"), 100.0 + fill("y")
    else:
        raise ValueError(family)
    f32 = lambda v: torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32))      # noqa: E731
    return f32(x), f32(y)


# ---------------------------------------------------------------------------------------------------------------------
# the restatement, one dtype throughout, with the explicit adjoint
# ---------------------------------------------------------------------------------------------------------------------
FAULTS = ("h_slip", "wrap_dropped", "end_central", "adjoint_ends", "mean_for_sum", "den_plain")


def _shift(v, s, axis, wrap=True):
    """v[i - s] along axis; without wrap: zero where i - s leaves the axis"""
    out = torch.roll(v, s, axis)
    if not wrap:
        out = out.clone()
        out.select(axis, 0 if s > 0 else v.shape[axis] - 1).zero_()
    return out


def diff(v, axis, h, fix, fault=None):
    """D_k v"""
    wrap = fault != "wrap_dropped"
    dv = (_shift(v, -1, axis, wrap) - _shift(v, 1, axis, wrap)) / (2.0 * h)
    if fix and fault != "end_central":
        n = v.shape[axis]
        dv = dv.clone()
        dv.select(axis, 0).copy_((v.select(axis, 1) - v.select(axis, 0)) / h)
        dv.select(axis, n - 1).copy_((v.select(axis, n - 1) - v.select(axis, n - 2)) / h)
    return dv


def diff_T(r, axis, h, fix, fault=None):
    """D_k^T r, written out: not autograd"""
    n = r.shape[axis]
    rt = r
    if fix and fault != "end_central":
        rt = r.clone()
        rt.select(axis, 0).zero_()
        rt.select(axis, n - 1).zero_()
    wrap = fault != "wrap_dropped"
    out = (_shift(rt, 1, axis, wrap) - _shift(rt, -1, axis, wrap)) / (2.0 * h)
    if fix and fault not in ("end_central", "adjoint_ends"):
        r0, rn = r.select(axis, 0) / h, r.select(axis, n - 1) / h
        out.select(axis, 0).sub_(r0)
        out.select(axis, 1).add_(r0)
        out.select(axis, n - 1).add_(rn)
        out.select(axis, n - 2).sub_(rn)
    return out


def reduce_all(planes, reduce_dims, reductions):
    if reduce_dims is None:
        return planes
    for dim, how in zip(reduce_dims, reductions):
        planes = planes.sum(dim=dim, keepdim=True) if how == "sum" else planes.mean(dim=dim, keepdim=True)
    return planes.squeeze()


def restated(x, y, d, h, dtype, order=1, relative=True, fix=None, reduce_dims=(0,), reductions=("sum",), g=None, fault=None):
    """{"value": the reduced loss, "planes": the per-plane tensor `lead`, "grad": d(sum(g * value))/dx (g = 1 when None)}, in
    `dtype` on the CPU.  The reduction's own adjoint is taken by autograd on the small per-plane tensor; the stencil's is the
    explicit one above."""
    assert fault is None or fault in FAULTS
    x, y = x.to(dtype), y.to(dtype)
    fix = (False,) * d if fix is None else tuple(fix)
    hs = [float(v) for v in h]
    if fault == "h_slip":
        hs[-1] *= 1.25
    axes = tuple(range(x.dim() - d, x.dim()))
    e = x - y
    num, den = (e * e).sum(axes), (y * y).sum(axes)
    q = e.clone()
    if order:
        for k, ax in enumerate(axes):
            de, dy = diff(e, ax, hs[k], fix[k], fault), diff(y, ax, hs[k], fix[k], fault)
            num = num + (de * de).sum(axes)
            if fault != "den_plain":
                den = den + (dy * dy).sum(axes)
            q = q + diff_T(de, ax, hs[k], fix[k], fault)
    vol = math.prod(hs)
    planes = (num / den).sqrt() if relative else (vol * num).sqrt()
    if fault == "mean_for_sum" and reduce_dims is not None:
        reductions = ["mean" if r == "sum" else "sum" for r in reductions]
    leaf = planes.detach().clone().requires_grad_(True)
    value = reduce_all(leaf, reduce_dims, reductions)
    value.backward(torch.ones_like(value) if g is None else torch.as_tensor(g, dtype=dtype).reshape(value.shape))
    live = num > 0
    safe = torch.where(live, num, torch.ones_like(num))
    coef = leaf.grad / (safe * den).sqrt() if relative else leaf.grad * math.sqrt(vol) / safe.sqrt()
    coef = torch.where(live, coef, torch.zeros_like(coef))
    return {"value": value.detach(), "planes": planes, "grad": coef.reshape(coef.shape + (1,) * d) * q}


def composed(x, y, d, h, order=1, relative=True, fix=None, reduce_dims=(0,), reductions=("sum",)):
    """the loss composed from torch operations (roll, slices, sums) in the dtype and on the device of its inputs,
    differentiable by autograd: what the explicit adjoint is checked against, and what tools/bench_sobolev_loss.py times the
    engine against.  Returns (value, planes)."""
    fix = (False,) * d if fix is None else tuple(fix)
    axes = tuple(range(x.dim() - d, x.dim()))
    e = x - y
    num, den = (e * e).sum(axes), (y * y).sum(axes)
    if order:
        for k, ax in enumerate(axes):
            num = num + (diff(e, ax, h[k], fix[k]) ** 2).sum(axes)
            den = den + (diff(y, ax, h[k], fix[k]) ** 2).sum(axes)
    planes = (num / den).sqrt() if relative else (math.prod(h) * num).sqrt()
    return reduce_all(planes, reduce_dims, reductions), planes


def autograd_reference(x, y, d, h, dtype, order=1, relative=True, fix=None, reduce_dims=(0,), reductions=("sum",), g=None):
    """`composed` in `dtype` on the CPU with autograd's gradient, in the form of `restated`"""
    x, y = x.to(dtype).clone().requires_grad_(True), y.to(dtype)
    value, planes = composed(x, y, d, h, order, relative, fix, reduce_dims, reductions)
    value.backward(torch.ones_like(value) if g is None else torch.as_tensor(g, dtype=dtype).reshape(value.shape))
    return {"value": value.detach(), "planes": planes.detach(), "grad": x.grad}


@functools.lru_cache(maxsize=64)
def references(family, shape, d, order=1, relative=True, fix=None, reduce_dims=(0,), reductions=("sum",), L=L_DEFAULT, h=None):
    """(x, y, h, ref64, ref32) of one case, computed once and shared; nobody writes into them"""
    x, y = make_inputs(family, shape, d)
    hs = uniform_h(shape, d, L if isinstance(L, float) else list(L)) if h is None else ([h] * d if isinstance(h, float) else list(h))
    kw = dict(order=order, relative=relative, fix=fix, reduce_dims=reduce_dims, reductions=reductions)
    return x, y, hs, restated(x, y, d, hs, torch.float64, **kw), restated(x, y, d, hs, torch.float32, **kw)


# ---------------------------------------------------------------------------------------------------------------------
# the judged quantities
# ---------------------------------------------------------------------------------------------------------------------
def worst_plane_err(a, ref64, d):
    """the largest relative L2 of one plane's gradient; a plane whose truth is all zero counts absolutely"""
    b = ref64.detach().to(torch.float64)
    a = a.detach().to(device="cpu", dtype=torch.float64).reshape(b.shape)
    axes = tuple(range(b.dim() - d, b.dim()))
    den = (b * b).sum(axes).sqrt()
    return float((((a - b) ** 2).sum(axes).sqrt() / torch.where(den > 0, den, torch.ones_like(den))).max())


def loss_rows(got, ref64, ref32, d, prefix=""):
    """judge_budget rows (name, err, err_ref32, floor) of got = {"value"[, "planes"][, "grad"]} against the float64
    restatement, the float32 one as the yardstick"""
    rows = [(prefix + "value", rel_err(got["value"].reshape(ref64["value"].shape), ref64["value"]), rel_err(ref32["value"], ref64["value"]), FLOOR)]
    if "planes" in got:
        rows.append((prefix + "planes", rel_err(got["planes"].reshape(ref64["planes"].shape), ref64["planes"]),
                     rel_err(ref32["planes"], ref64["planes"]), FLOOR))
    if "grad" in got:
        rows += [(prefix + "dx", rel_err(got["grad"], ref64["grad"]), rel_err(ref32["grad"], ref64["grad"]), FLOOR),
                 (prefix + "dx worst plane", worst_plane_err(got["grad"], ref64["grad"], d), worst_plane_err(ref32["grad"], ref64["grad"], d), FLOOR)]
    capped = [name for name, _, ref, _ in rows if not ref < CAP]
    assert not capped, f"float32 yardstick at or above {CAP}: {capped}"
    return rows


def combo_name(family, order, relative, fix):
    return f"{family:6s} {'H1' if order else 'Lp'} {'rel' if relative else 'abs'} fix={''.join('1' if f else '0' for f in fix)} "


def combos(d):
    """(order, relative, fix) of every form: H1 in every boundary mode, Lp (which has none) once"""
    return [(1, rel, fix) for rel in (True, False) for fix in fix_modes(d)] + [(0, rel, (False,) * d) for rel in (True, False)]
