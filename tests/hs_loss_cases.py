"""What the spectral Sobolev loss (csrc/k_hs_loss.h, functional.hs_loss, libs.utilities3.HsLoss) is held to: a helper module,
not a conftest.

`restated` states HsLoss of the reference (libs/utilities3.py:339-405) in one dtype with EXACT weights and the explicit
adjoint; in float64 it is the truth, in float32 the yardstick.  tests/golden/hs_loss_small.npz holds the reference's own
float32 losses and gradients and ties the restatement to it (tests/test_hs_loss_host.py).

    x, y (B, N, N, *rest) -> (B, N, N, C);  e = x - y;  E = fftn(e, dim=[1, 2]), Y = fftn(y, dim=[1, 2])
    r2 = kx^2 + ky^2 of |k|, k = [0 .. n/2-1, -n/2 .. -1] (the Nyquist index carries n/2);  w2 = (1, a[0]^2, a[1]^2)
    num_j = w2[j] sum_{kx,ky,c} r2^j |E|^2,  den_j = w2[j] sum r2^j |Y|^2,  j <= min(k, 2)
    ungrouped: v_b = sqrt(sum_j num_j) / sqrt(sum_j den_j)         grouped: v_b = (sum_j sqrt(num_j / den_j)) / (k + 1)
    value = mean_b v_b | sum_b v_b | v
    dx = n^2 Re(ifftn(Wc E)),  Wc = sum_j c_j w2[j] r2^j,  c_j = g_b / sqrt(num den)  or  g_b / ((k + 1) sqrt(num_j den_j)),
         0 where that num is 0;  g_b = the upstream gradient of v_b

Input families, built in float64 from oracle.detfill and rounded once:
  white    x uniform +-1, y = uniform +-1 + 0.3
  near     x = y (1 + 1e-3 fill), y as in white
  smooth   the modes (p, q), p, q = 0 .. 3 without (0, 0), with amplitudes fill / (p^2 + q^2) and random phases, per field
  big      white x 1e4          small    white x 1e-4

Criterion: tests.judging.judge_budget (slack BUDGET_SLACK) with the floor of tests/sobolev_cases.py, FLOOR = 2e-6.  No row is
ever left out.  The smooth family under the |k|^4 weight is ill-conditioned by construction: the truth's own gradient there is
the float32 rounding of the INPUTS amplified by up to (n^2 / 2)^2, so the float32 yardstick of dx reaches 1e-4 at n = 32 and
3.8e-2 at (1, 128, 128, 2) and those rows compare two draws of rounding noise; they are judged like every other row and stand in the
log with their yardstick.  Every figure goes to profiles/r24_hs_loss_errors.txt before anything is asserted."""
import functools
import math
import os

import numpy as np
import torch

from oracle.detfill import name_seed, unit_fill
from tests.judging import SectionLog, rel_err
from tests.sobolev_cases import FLOOR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
LOG = SectionLog(os.path.join(ROOT, "profiles", "r24_hs_loss_errors.txt"))
GRIDS = (32, 64, 128)
FAMILIES = ("white", "near", "smooth", "big", "small")
# (k, a, group): the default; two weighted orders; the same grouped; the plain relative L2 as a group of one; a non-unit weight
# grouped; k = 3, where only three terms exist and the grouped divisor is still k + 1
FORMS = ((1, None, False), (2, (0.5, 0.25), False), (2, (0.5, 0.25), True), (0, None, True), (1, (2.0,), True), (3, None, False),
         (3, None, True))
REDUCTIONS = ("mean", "sum", None)
# one plane; three samples; an odd channel count (a pair and a single); trailing dimensions that fold; the other two grids
SHAPES = ((1, 32, 32), (3, 32, 32), (2, 32, 32, 3), (2, 32, 32, 2, 2), (2, 64, 64), (1, 128, 128, 2))
GOLDEN_SHAPE = (2, 32, 32, 2)
GOLDEN_SCALES = {"x": 1.0, "y": 1.0}


def shape_id(shape):
    return "x".join(str(n) for n in shape)


def form_id(k, a, group):
    return f"k{k}_a{'default' if a is None else '-'.join(str(v) for v in a)}_{'grouped' if group else 'plain'}"


def upstream(reduce, B):
    """the upstream gradient a reduction is exercised with: the default under mean, 0.37 under sum, a non-uniform (B,) vector
    on the per-sample values"""
    return {"mean": None, "sum": 0.37, None: [0.5 + 0.3 * b * (-1) ** b for b in range(B)]}[reduce]


def golden_inputs():
    """the fixture's inputs, rebuilt from their fill names and scales"""
    f = lambda name: GOLDEN_SCALES[name] * unit_fill(GOLDEN_SHAPE, name_seed(f"hs.golden.{name}"))      # noqa: E731
    return tuple(torch.from_numpy(np.ascontiguousarray(f(n), dtype=np.float32)) for n in ("x", "y"))


@functools.lru_cache(maxsize=None)
def make_inputs(family, shape):
    """(x, y) float32 on the CPU"""
    tag = f"hs.{family}.{shape_id(shape)}"
    fill = lambda name: unit_fill(shape, name_seed(f"{tag}.{name}"))      # noqa: E731
    B, n, lead = shape[0], shape[1], (shape[0],) + (1, 1) + tuple(shape[3:])

    def smooth(name):
        i = np.arange(n).reshape((1, n, 1) + (1,) * (len(shape) - 3))
        j = np.arange(n).reshape((1, 1, n) + (1,) * (len(shape) - 3))
        v = np.zeros(shape)
        for p in range(0, 4):
            for q in range(0, 4):
                if p + q == 0:
                    continue
                amp = unit_fill((B,) + tuple(shape[3:]), name_seed(f"{tag}.{name}.a{p}{q}")).reshape(lead) / (p * p + q * q)
                ph = math.pi * unit_fill((B,) + tuple(shape[3:]), name_seed(f"{tag}.{name}.p{p}{q}")).reshape(lead)
                v = v + amp * np.cos(2 * math.pi * (p * i + q * j) / n + ph)
        return v
    if family in ("white", "big", "small"):
        s = {"white": 1.0, "big": 1e4, "small": 1e-4}[family]
        x, y = s * fill("x"), s * (fill("y") + 0.3)
    elif family == "near":
        y = fill("y") + 0.3
        x = y * (1.0 + 1e-3 * fill("x"))
    elif family == "smooth":
        x, y = smooth("x"), smooth("y")
    else:
        raise ValueError(family)
    f32 = lambda v: torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32))      # noqa: E731
    return f32(x), f32(y)


# ---------------------------------------------------------------------------------------------------------------------
# the restatement, one dtype throughout, with the explicit adjoint
# ---------------------------------------------------------------------------------------------------------------------
FAULTS = ("nyquist_signed", "bin_natural", "divisor_terms", "mean_for_sum", "a_unsquared", "den_plain")


def wave_r2(n, dtype, fault=None):
    """r2 (1, n, n, 1) of the absolute wave numbers, exact in either dtype (integers below 2^24)"""
    k = torch.cat((torch.arange(0, n // 2), torch.arange(-(n // 2), 0))).abs().to(dtype)
    if fault == "nyquist_signed":           # the Nyquist row dropped instead of carrying n/2
        k[n // 2] = 0
    if fault == "bin_natural":              # the weight of the natural position on a bit-reversed spectrum
        bits = n.bit_length() - 1
        k = k[[int(format(i, f"0{bits}b")[::-1], 2) for i in range(n)]]
    return (k.reshape(1, n, 1, 1) ** 2 + k.reshape(1, 1, n, 1) ** 2)


def spectral_sums(x, y, dtype, fault=None):
    """what every form is made of: E and, per sample, sum r2^j |E|^2 and sum r2^j |Y|^2 for j = 0, 1, 2, in `dtype`"""
    B, n = x.shape[0], x.shape[1]
    assert x.shape[2] == n
    x, y = x.to(dtype).reshape(B, n, n, -1), y.to(dtype).reshape(B, n, n, -1)
    E, Y = torch.fft.fftn(x - y, dim=[1, 2]), torch.fft.fftn(y, dim=[1, 2])
    r2 = wave_r2(n, dtype, fault)
    pe, py = E.real ** 2 + E.imag ** 2, Y.real ** 2 + Y.imag ** 2
    return {"E": E, "r2": r2, "n": n, "Se": torch.stack([(r2 ** j * pe).sum((1, 2, 3)) for j in range(3)], 1),
            "Sy": torch.stack([(r2 ** j * py).sum((1, 2, 3)) for j in range(3)], 1), "dtype": dtype}


def reduce_values(v, reduce):
    return v.mean() if reduce == "mean" else v.sum() if reduce == "sum" else v


def from_sums(s, shape, k=1, a=None, group=False, reduce="mean", g=None, fault=None):
    """{"value": the reduced loss, "samples": the (B,) values, "grad": d(sum(g * value))/dx (g = 1 when None)}.  The product
    num den is taken as sqrt(num) sqrt(den): at inputs of 1e4 it leaves float32's range"""
    dtype = s["dtype"]
    a = [1.0] * k if a is None else list(a)
    terms = min(k, 2) + 1
    w2 = torch.tensor([1.0] + [float(v) ** (1 if fault == "a_unsquared" else 2) for v in a[:terms - 1]], dtype=dtype)
    num, den = s["Se"][:, :terms] * w2, s["Sy"][:, :terms] * w2
    if fault == "den_plain":                # the target's norm without the derivative terms
        den = den * torch.tensor([1.0, 0.0, 0.0][:terms], dtype=dtype)
    div = float(terms if fault == "divisor_terms" else k + 1)
    if group:
        samples = (num.sqrt() / den.sqrt()).sum(1) / div
    else:
        samples = num.sum(1).sqrt() / den.sum(1).sqrt()
    leaf = samples.detach().clone().requires_grad_(True)
    how = {"mean": "sum", "sum": "mean"}.get(reduce, reduce) if fault == "mean_for_sum" else reduce
    value = reduce_values(leaf, how)
    value.backward(torch.ones_like(value) if g is None else torch.as_tensor(g, dtype=dtype).reshape(value.shape))
    gb = leaf.grad
    if group:
        live = num > 0
        c = torch.where(live, gb[:, None] / (div * torch.where(live, num, torch.ones_like(num)).sqrt() * den.sqrt()), torch.zeros_like(num))
    else:
        tn, td = num.sum(1), den.sum(1)
        live = tn > 0
        c = torch.where(live, gb / (torch.where(live, tn, torch.ones_like(tn)).sqrt() * td.sqrt()), torch.zeros_like(tn))[:, None].expand(-1, terms)
    Wc = sum((c[:, j] * w2[j]).reshape(-1, 1, 1, 1) * s["r2"] ** j for j in range(terms))
    grad = torch.fft.ifftn(Wc * s["E"], dim=[1, 2]).real * float(s["n"] * s["n"])
    return {"value": value.detach(), "samples": samples, "grad": grad.reshape(shape)}


def restated(x, y, dtype, k=1, a=None, group=False, reduce="mean", g=None, fault=None):
    return from_sums(spectral_sums(x, y, dtype, fault), tuple(x.shape), k, a, group, reduce, g, fault)


def composed(x, y, k=1, a=None, group=False, reduce="mean"):
    """the reference's own formula composed from torch operations (torch.fft.fftn, complex products, torch.norm) in the dtype and
    on the device of its inputs, differentiable by autograd: what the explicit adjoint is checked against, and what
    tools/bench_hs_loss.py times the engine against.  The weights are built in x's dtype (the reference: always float32)."""
    B, n = x.shape[0], x.shape[1]
    a = [1.0] * k if a is None else list(a)
    x, y = x.reshape(B, n, n, -1), y.reshape(B, n, n, -1)
    r2 = wave_r2(n, x.dtype).to(x.device)
    xf, yf = torch.fft.fftn(x, dim=[1, 2]), torch.fft.fftn(y, dim=[1, 2])

    def rel(u, v):
        return torch.norm(u.reshape(B, -1) - v.reshape(B, -1), 2, 1) / torch.norm(v.reshape(B, -1), 2, 1)
    if not group:
        w = torch.ones_like(r2)
        if k >= 1:
            w = w + a[0] ** 2 * r2
        if k >= 2:
            w = w + a[1] ** 2 * r2 ** 2
        w = w.sqrt()
        v = rel(xf * w, yf * w)
    else:
        v = rel(xf, yf)
        if k >= 1:
            w = a[0] * r2.sqrt()
            v = v + rel(xf * w, yf * w)
        if k >= 2:
            w = a[1] * r2
            v = v + rel(xf * w, yf * w)
        v = v / (k + 1)
    return reduce_values(v, reduce), v


def autograd_reference(x, y, dtype, k=1, a=None, group=False, reduce="mean", g=None):
    """`composed` in `dtype` on the CPU with autograd's gradient, in the form of `restated`"""
    x, y = x.to(dtype).clone().requires_grad_(True), y.to(dtype)
    value, samples = composed(x, y, k, a, group, reduce)
    value.backward(torch.ones_like(value) if g is None else torch.as_tensor(g, dtype=dtype).reshape(value.shape))
    return {"value": value.detach(), "samples": samples.detach(), "grad": x.grad}


@functools.lru_cache(maxsize=64)
def sums_of(family, shape):
    """(x, y, float64 sums, float32 sums) of one input, computed once and shared by every form; nobody writes into them"""
    x, y = make_inputs(family, shape)
    return x, y, spectral_sums(x, y, torch.float64), spectral_sums(x, y, torch.float32)


def references(family, shape, k=1, a=None, group=False, reduce="mean", g=None):
    """(x, y, ref64, ref32) of one case"""
    x, y, s64, s32 = sums_of(family, shape)
    return x, y, from_sums(s64, shape, k, a, group, reduce, g), from_sums(s32, shape, k, a, group, reduce, g)


# ---------------------------------------------------------------------------------------------------------------------
# the judged quantities
# ---------------------------------------------------------------------------------------------------------------------
def worst_sample_err(a, ref64):
    """the largest relative L2 of one sample's gradient; a sample whose truth is all zero counts absolutely"""
    b = ref64.detach().to(torch.float64)
    a = a.detach().to(device="cpu", dtype=torch.float64).reshape(b.shape)
    axes = tuple(range(1, b.dim()))
    den = (b * b).sum(axes).sqrt()
    return float((((a - b) ** 2).sum(axes).sqrt() / torch.where(den > 0, den, torch.ones_like(den))).max())


def loss_rows(got, ref64, ref32, prefix=""):
    """judge_budget rows (name, err, err_ref32, floor) of got = {"value"[, "grad"]} against the float64 restatement, the
    float32 one as the yardstick; "value" is the reduced loss or, without a reduction, the (B,) values"""
    rows = [(prefix + "value", rel_err(got["value"].reshape(ref64["value"].shape), ref64["value"]), rel_err(ref32["value"], ref64["value"]), FLOOR)]
    if "grad" in got:
        rows += [(prefix + "dx", rel_err(got["grad"], ref64["grad"]), rel_err(ref32["grad"], ref64["grad"]), FLOOR),
                 (prefix + "dx worst sample", worst_sample_err(got["grad"], ref64["grad"]), worst_sample_err(ref32["grad"], ref64["grad"]), FLOOR)]
    return rows


def combo_name(family, k, a, group, reduce):
    return f"{family:6s} {form_id(k, a, group):28s} {str(reduce):4s} "


# ---------------------------------------------------------------------------------------------------------------------
# single cosine modes and their closed form
# ---------------------------------------------------------------------------------------------------------------------
def mode_pairs(n):
    return ((0, 0), (1, 0), (0, 1), (n // 2, n // 2), (n // 2 - 1, 3), (n - 1, 0))


def cosine_mode(n, p, q, amp):
    """amp cos(2 pi (p i + q j) / n) on the n x n grid, float64"""
    i, j = np.arange(n).reshape(n, 1), np.arange(n).reshape(1, n)
    return amp * np.cos(2 * math.pi * (p * i + q * j) / n)


def mode_weight(n, p, q, k, a):
    """(W, energy) of the mode: W = 1 + a0^2 |k|^2 + a1^2 |k|^4 at (p, q) and sum |F cos|^2 / n^4 - 1/2 from the two bins
    (p, q), (-p, -q), 1 where they are one bin"""
    kp, kq = min(p, n - p), min(q, n - q)
    r2 = float(kp * kp + kq * kq)
    a = [1.0] * k if a is None else list(a)
    W = 1.0 + (a[0] ** 2 * r2 if k >= 1 else 0.0) + (a[1] ** 2 * r2 * r2 if k >= 2 else 0.0)
    single = (2 * p) % n == 0 and (2 * q) % n == 0
    return W, (1.0 if single else 0.5)


def mode_loss(n, pq_e, amp_e, pq_y, amp_y, k, a):
    """the ungrouped loss of e = one mode, y = one mode: amplitude ratio x sqrt(W(p, q) / W(p', q')) (x the bin-count factor)"""
    We, ce = mode_weight(n, *pq_e, k, a)
    Wy, cy = mode_weight(n, *pq_y, k, a)
    return (amp_e / amp_y) * math.sqrt(We * ce / (Wy * cy))
