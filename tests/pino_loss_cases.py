"""What the PINO residual loss (k_pino_loss.h, k_pino_loss2.h, functional.pino_loss) is held to: the input families, the
float64 / float32 references, a float32 restatement of the kernels' arithmetic, the comparison and the error table.  Shared by
tests/test_pino_loss_gpu.py (the HIP kernels) and tests/test_pino_loss_reference.py (the same cases and the same comparison on
the CPU, the restatement standing in for the engine, and five planted faults that must be refused).

Criterion (tests/judging.py::accept): with err against oracle/pino_loss_oracle.py in float64 on float64 copies of the
same float32 inputs,   err_engine == 0 or err_engine < max(FLOOR, BUDGET_SLACK * err_ref32),   err_ref32 being the error of
the same oracle in float32 on the CPU.  FLOOR = 2e-6 (the gate-field floor) for every quantity; a row is judged only where
err_ref32 < CAP = 0.1, and only the rows of the floor family steady(0) may be above it (there they are logged).

Quantities: the stored residual Du - f (the fifth field array of the workspace, read by stored_field) as relative L2 over
everything, as the worst relative L2 of one (sample, time level) plane and as max |e| / rms; loss_f against the float64 norm
of the engine's OWN stored field (the reduction alone; yardstick: torch.norm in float32 of that field), loss_f against the
float64 oracle (logged: the triangle inequality bounds it by the field error), loss_ic, and dL/du of
IC_WEIGHT * loss_ic + loss_f overall and as the worst single time level.  The gradient's yardstick is ref32n, the float32
oracle with its two norms accumulated in float64: torch's float32 norm over 2 M elements is 3e-5 low by itself, which is an
error of the reference's reduction and not a budget for the field arithmetic; the error of the plain float32 oracle is logged
beside it.  Every row goes to the file $PINO_LOSS_ERROR_LOG names, in the format of the step-tail table."""
import functools
import math

import numpy as np
import torch

from oracle import pino_loss_oracle as P
from oracle.detfill import fill_named, name_seed, unit_fill
from tests.judging import BUDGET_SLACK, RowLog, accept, rel_err  # noqa: F401  (the floor test applies the slack to loss_f itself)
from tests.step_tail_cases import FLOOR_GATE, same_bits  # noqa: F401  (same_bits: re-exported to the tests)

FLOOR = FLOOR_GATE
CAP = 0.1                                   # a float32 reference further than this from float64 measures nothing
ROWS = RowLog("PINO_LOSS_ERROR_LOG")
VISCS = (1.0 / 180.0, 1.0 / 395.0, 1.0 / 40.0)
IC_WEIGHT, T_INTERVAL = 5.0, 0.5
PINO_CHUNK = 64                             # fno_abi.hip kPinoChunk: planes per pass of the slab kernels

BUDGET_SHAPES = ((32, 3, 3), (64, 2, 5), (128, 2, 4), (256, 2, 4))                    # (n, B, nt)
# the second near-steady row is delta = 1e-2, raised to 3e-2 at n = 256: at 1e-2 the float32 oracle's own gradient is 0.106 from
# float64 there (0.110 at its worst time level), above the cap under which a row is judged
STEADY_SMALL_DELTA = {32: 1e-2, 64: 1e-2, 128: 1e-2, 256: 3e-2}


def budget_families(n):
    return (("white", None), ("smooth", None), ("steady", 1e-1), ("steady", STEADY_SMALL_DELTA[n]))


SLAB_SHAPES = ((2, 34), (1, 67), (2, 35), (3, 45))                                    # (B, nt) at n = 256: 64, 65, 66, 129 planes
SLAB_T_INTERVAL = 0.37
GRIDS = (32, 64, 128, 256)


def case_name(family, delta, n, B, nt, t_interval=T_INTERVAL):
    fam = family if delta is None else f"{family}({delta:g})"
    return f"pino {fam} n={n} B={B} nt={nt} t={t_interval:g}"


# ---------------------------------------------------------------------------------------------------------------------
# input families: deterministic, built in float64, rounded once to float32
# ---------------------------------------------------------------------------------------------------------------------
def _smooth64(tag, B, n, nt):
    """three fields of amplitude spectrum |k|^-3 and hashed phases per sample, each normalised to max 1 and multiplied by its
    own cosine in time"""
    k = P.wavenumbers(n, dtype=torch.float64).numpy()
    k2 = k[:, None] ** 2 + k[None, :] ** 2
    k2[0, 0] = 1.0
    amp = k2 ** -1.5
    amp[0, 0] = 0.0
    tau = np.arange(nt, dtype=np.float64) / (nt - 1)
    out = np.zeros((B, n, n, nt))
    for b in range(B):
        for j in range(3):
            phase = unit_fill((n, n), name_seed(f"{tag}.smooth.{b}.{j}"))
            g = np.real(np.fft.ifft2(amp * np.exp(1j * math.pi * phase)))
            g /= np.abs(g).max()
            out[b] += g[:, :, None] * np.cos(math.pi * (j + 1) * tau + 0.7 * j + b)[None, None, :]
    return out


def make_inputs(family, B, n, nt, delta=None):
    """{"u" (B, n, n, nt), "u0" (B, n, n), "f" (1, n, n, 1): the shipped forcing -4 cos 4y, "visc" (B,)}, float32 on the CPU.
    u0 is independent white noise for white / const / zero and u[..., 0] + 0.1 white otherwise."""
    assert B <= len(VISCS)
    tag = f"pinoloss.{family}.{delta}.{B}.{n}.{nt}"
    visc = torch.tensor(VISCS[:B], dtype=torch.float32)
    white0 = fill_named(tag + ".u0", (B, n, n), 1.0, dtype=np.float64)
    if family == "white":
        u, u0 = fill_named(tag + ".u", (B, n, n, nt), 1.0, dtype=np.float64), white0
    elif family == "smooth":
        u = _smooth64(tag, B, n, nt)
        u0 = u[..., 0] + 0.1 * white0
    elif family == "steady":
        y = np.arange(n, dtype=np.float64) * (2.0 * math.pi / n)                       # y is dim 2
        base = -np.cos(4.0 * y)[None, None, :, None] / (4.0 * visc.double().numpy()[:, None, None, None])
        u = np.broadcast_to(base, (B, n, n, nt)).copy()
        if delta:
            u += delta * _smooth64(tag, B, n, nt)
        u0 = u[..., 0] + 0.1 * white0
    elif family == "const":
        # multiples of 1/16 in [-2, 2): every sum of the transforms is exact, and so is nu * c in float64 (const_expected)
        c = np.round(unit_fill((B, nt), name_seed(tag + ".c")) * 32.0) / 16.0
        u, u0 = np.broadcast_to(c[:, None, None, :], (B, n, n, nt)).copy(), white0
    elif family == "zero":
        u, u0 = np.zeros((B, n, n, nt)), white0
    else:
        raise ValueError(family)
    return {"u": torch.from_numpy(u.astype(np.float32)), "u0": torch.from_numpy(u0.astype(np.float32)),
            "f": P.forcing(n), "visc": visc}


# ---------------------------------------------------------------------------------------------------------------------
# references: the oracle in float64 (ref64), in float32 (ref32), in float32 with float64 norms (ref32n)
# ---------------------------------------------------------------------------------------------------------------------
def lp_rel_mean_n(x, y):
    """oracle.lp_rel_mean with only its two norms accumulated in float64"""
    B = x.shape[0]
    d = torch.norm((x.reshape(B, -1) - y.reshape(B, -1)).double(), 2, 1).to(x.dtype)
    return torch.mean(d / torch.norm(y.reshape(B, -1).double(), 2, 1).to(x.dtype))


FAULTS = ("nonlinear", "nyquist_row", "visc_chunk", "last_level_adjoint", "dt_slip")


def faulty_residual(w, visc, t_interval, fault):
    """oracle.ns_vorticity_residual restated with one planted fault:
      nonlinear           u . grad(w) times 1.001
      nyquist_row         the row kx = -n/2 dropped from u_y
      visc_chunk          planes (b (T - 2) + t - 1) >= PINO_CHUNK take visc[0]
      last_level_adjoint  the last time level's share of the central difference carries no gradient
      dt_slip             w_t times T / (T - 1)"""
    assert fault in FAULTS
    B, n, _, nt = w.shape
    k = P.wavenumbers(n, w.device, w.dtype)
    kx, ky = k.reshape(1, n, 1, 1), k.reshape(1, 1, n, 1)
    lap = (kx ** 2 + ky ** 2).clone()
    lap[0, 0, 0, 0] = 1.0
    w_h = torch.fft.fft2(w, dim=[1, 2])
    psi_h = w_h / lap
    half = n // 2 + 1

    def back(spec):
        return torch.fft.irfft2(spec[:, :, :half], dim=[1, 2])
    uy_h = -1j * kx * psi_h
    if fault == "nyquist_row":
        keep = torch.ones(1, n, 1, 1, dtype=w.dtype)
        keep[0, n // 2] = 0.0
        uy_h = uy_h * keep
    ux, uy, wx, wy, wlap = back(1j * ky * psi_h), back(uy_h), back(1j * kx * w_h), back(1j * ky * w_h), back(-lap * w_h)
    nl = ux * wx + uy * wy
    if fault == "nonlinear":
        nl = nl * 1.001
    nu = visc.reshape(B, 1, 1, 1).repeat(1, 1, 1, nt)
    if fault == "visc_chunk":
        plane = torch.arange(B).reshape(B, 1) * (nt - 2) + torch.arange(nt).reshape(1, nt) - 1
        nu = torch.where((plane >= PINO_CHUNK).reshape(B, 1, 1, nt), visc[0], nu)
    hi = w[..., 2:]
    if fault == "last_level_adjoint":
        hi = torch.cat([w[..., 2:-1], w[..., -1:].detach()], -1)
    wt = (hi - w[..., :-2]) / (2 * (t_interval / (nt - 1)))
    if fault == "dt_slip":
        wt = wt * (nt / (nt - 1))
    return wt + (nl - nu * wlap)[..., 1:-1]


def planes_of(du):
    """(B, n, n, T - 2) of the oracle -> (B, T - 2, n, n), the engine's plane order"""
    return du.detach().permute(0, 3, 1, 2).contiguous()


def oracle_eval(inp, dtype, t_interval=T_INTERVAL, g_ic=IC_WEIGHT, g_f=1.0, norms64=False, fault=None, grad=True):
    """{"loss_ic", "loss_f" (0-dim), "field" = Du - f (B, T - 2, n, n), "grad" = d(g_ic loss_ic + g_f loss_f)/du} of
    oracle/pino_loss_oracle.py in `dtype` on copies of the float32 inputs"""
    u = inp["u"].to(dtype).clone().requires_grad_(grad)
    u0, f, visc = inp["u0"].to(dtype), inp["f"].to(dtype), inp["visc"].to(dtype)
    B, n, _, nt = u.shape
    rel = lp_rel_mean_n if norms64 else P.lp_rel_mean
    du = P.ns_vorticity_residual(u, visc, t_interval) if fault is None else faulty_residual(u, visc, t_interval, fault)
    f_rep = f.repeat(B, 1, 1, nt - 2)
    loss_ic, loss_f = rel(u[..., 0], u0), rel(du, f_rep)
    out = {"loss_ic": loss_ic.detach(), "loss_f": loss_f.detach(), "field": planes_of(du - f_rep)}
    if grad:
        (g_ic * loss_ic + g_f * loss_f).backward()
        out["grad"] = u.grad
    return out


@functools.lru_cache(maxsize=4)
def references(family, delta, n, B, nt, t_interval=T_INTERVAL):
    """(inputs, ref64, ref32, ref32n) of one case, computed once and shared; nobody writes into them"""
    inp = make_inputs(family, B, n, nt, delta)
    return (inp, oracle_eval(inp, torch.float64, t_interval), oracle_eval(inp, torch.float32, t_interval),
            oracle_eval(inp, torch.float32, t_interval, norms64=True))


# ---------------------------------------------------------------------------------------------------------------------
# the kernels' arithmetic in float32 numpy (forward): radix-2 DIF forward, DIT inverse, float32 twiddles, multipliers at
# full-grid indices with the Hermitian extension, 1 / n^2 after the inverse.  No fused multiply-adds.
# ---------------------------------------------------------------------------------------------------------------------
def _brev(n):
    bits = n.bit_length() - 1
    return np.array([int(format(i, f"0{bits}b")[::-1], 2) for i in range(n)])


def _fft_last(re, im, inverse):
    """in place along the last axis (k_pino_loss.h fft_lines): forward natural -> bit-reversed, inverse the other way"""
    n = re.shape[-1]
    ang = -2.0 * np.arange(n // 2, dtype=np.float64) / n
    twr, twi = np.cos(math.pi * ang).astype(np.float32), np.sin(math.pi * ang).astype(np.float32)
    j = np.arange(n // 2)
    hs = [n >> (s + 1) for s in range(n.bit_length() - 1)]
    for h in (hs[::-1] if inverse else hs):
        pos = j & (h - 1)
        i0 = ((j - pos) << 1) + pos
        i1 = i0 + h
        wr, wi = twr[pos * (n // 2 // h)], twi[pos * (n // 2 // h)]
        ar, ai, br, bi = re[..., i0], im[..., i0], re[..., i1], im[..., i1]
        if not inverse:
            dr, di = ar - br, ai - bi
            re[..., i0], im[..., i0] = ar + br, ai + bi
            re[..., i1], im[..., i1] = dr * wr - di * wi, dr * wi + di * wr
        else:
            wi = -wi
            cr, ci = br * wr - bi * wi, br * wi + bi * wr
            re[..., i0], im[..., i0] = ar + cr, ai + ci
            re[..., i1], im[..., i1] = ar - cr, ai - ci


def _multipliers(n):
    """pino_mult at every full-grid index, natural order: five (re, im) pairs of (n, n) float32"""
    ix, iy = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    ext = iy > n // 2
    jx, jy = np.where(ext, (n - ix) & (n - 1), ix), np.where(ext, n - iy, iy)
    kx = np.where(jx < n // 2, jx, jx - n).astype(np.float32)
    ky = np.where(jy < n // 2, jy, jy - n).astype(np.float32)
    lap = kx * kx + ky * ky
    lap[(jx == 0) & (jy == 0)] = 1.0
    sign = np.where(ext, np.float32(-1.0), np.float32(1.0))
    zero = np.zeros((n, n), np.float32)
    return [(zero, sign * (ky / lap)), (zero, sign * kx), (zero, sign * (-kx / lap)), (zero, sign * ky), (-lap, zero)]


def restated_forward(inp, t_interval=T_INTERVAL, slab=None):
    """{"loss_ic", "loss_f", "field"} by the forward kernels' arithmetic.  slab: the inverse runs x then y (k_pino2_cols_fwd,
    k_pino2_rows_inv) instead of y then x (fft2_grid); default: as the engine routes the grid, slabs at n = 256."""
    u, u0 = inp["u"].numpy(), inp["u0"].numpy()
    f, visc = inp["f"].numpy().reshape(inp["u"].shape[1:3]), inp["visc"].numpy()
    B, n, _, nt = u.shape
    slab = (n == 256) if slab is None else slab
    f32 = np.float32
    inv2dt, inv_n2 = f32((nt - 1) / (2.0 * t_interval)), f32(1.0 / (n * n))
    w = np.ascontiguousarray(np.moveaxis(u, 3, 1))                                       # (B, nt, n, n)
    acc = (w[:, 2:] - w[:, :-2]) * inv2dt
    re, im = w[:, 1:-1].copy(), np.zeros((B, nt - 2, n, n), f32)
    _fft_last(re, im, False)                                                            # along y, then along x
    _fft_last(re.swapaxes(-1, -2), im.swapaxes(-1, -2), False)
    br = _brev(n)
    vals = []
    for mr, mi in _multipliers(n):
        mr, mi = mr[br][:, br], mi[br][:, br]
        gr, gi = mr * re - mi * im, mr * im + mi * re
        for axis_swapped in ((True, False) if slab else (False, True)):
            if axis_swapped:
                _fft_last(gr.swapaxes(-1, -2), gi.swapaxes(-1, -2), True)
            else:
                _fft_last(gr, gi, True)
        vals.append(gr * inv_n2)
    nu = visc.astype(f32).reshape(B, 1, 1, 1)
    acc = acc + vals[0] * vals[1]
    acc = acc + vals[2] * vals[3]
    acc = acc + (-nu) * vals[4]
    r = acc - f
    assert r.dtype == np.float32
    fnorm = np.sqrt(np.sum(f * f, dtype=f32) * f32(nt - 2))
    lf = lic = f32(0.0)
    for b in range(B):
        sf = f32(0.0)
        for t in range(nt - 2):
            sf = sf + np.sum(r[b, t] * r[b, t], dtype=f32)
        d = u[b, :, :, 0] - u0[b]
        lf = lf + np.sqrt(sf) / fnorm
        lic = lic + np.sqrt(np.sum(d * d, dtype=f32)) / np.sqrt(np.sum(u0[b] * u0[b], dtype=f32))
    return {"loss_ic": torch.tensor(lic / f32(B)), "loss_f": torch.tensor(lf / f32(B)), "field": torch.from_numpy(r)}


def const_expected(inp, t_interval):
    """The stored field for a const-in-space input, bit for bit.  Every butterfly difference is an exact zero, so the
    spectrum is the mean mode alone; the four velocity / gradient multipliers are zero there, but the reference sets the
    Laplacian's (0, 0) entry to 1 (diff_control_env.py:22, 29), so lap(w) comes back as exactly -c and the kernel forms
        fma(-nu, -c, fl((u[t+1] - u[t-1]) * float32((T - 1) / (2 t_interval)))) - f.
    c is a multiple of 1/16 below 2 and nu has 24 bits: nu c is exact in float64, its sum with w_t too (the exponents are
    less than 2^20 apart), so one rounding to float32 is the fused multiply-add."""
    u, f, visc = inp["u"].numpy(), inp["f"].numpy().reshape(inp["u"].shape[1:3]), inp["visc"].numpy()
    B, n, _, nt = u.shape
    c = u[:, 0, 0, :]                                                                   # (B, nt) float32
    wt = (c[:, 2:] - c[:, :-2]) * np.float32((nt - 1) / (2.0 * t_interval))
    assert wt.dtype == np.float32
    acc = (wt.astype(np.float64) + visc.astype(np.float64)[:, None] * c[:, 1:-1].astype(np.float64)).astype(np.float32)
    return torch.from_numpy(acc[:, :, None, None] - f[None, None])


# ---------------------------------------------------------------------------------------------------------------------
# reading the engine's stored field, and the comparison
# ---------------------------------------------------------------------------------------------------------------------
def stored_field(loss_f, B, n, nt, copy=True):
    """Du - f as the forward call behind `loss_f` left it: carve_pino (fno_abi.hip) puts the five field arrays of
    B (T - 2) n^2 floats first in the workspace - u_x, w_x, u_y, w_y, residual - and _PinoLossFn saves the workspace last.
    The one place in the tests that knows this.  Returns (B, T - 2, n, n): a copy, or with copy=False a view of the
    workspace itself (to look at it again after the backward passes have released the graph)."""
    ws = loss_f.grad_fn.saved_tensors[-1]
    assert ws.dtype == torch.uint8
    np_ = B * (nt - 2) * n * n
    view = ws[16 * np_:20 * np_].view(torch.float32).reshape(B, nt - 2, n, n)
    return view.clone() if copy else view


def judge(case, tensor, err_engine, err_ref32, floor=FLOOR, who="engine", log_only=False):
    """One row of the error table (tests/step_tail_cases.py::judge's format) and a description of the failure, or None.
    log_only: recorded, never judged (loss_f against the oracle, the plain float32 oracle's gradient error, and every row
    of the floor family).  Anywhere else a reference error of CAP or more is a failure by itself."""
    capped = not err_ref32 < CAP
    if log_only:
        verdict, bad = "logged", None
    elif capped:
        verdict, bad = "FAIL", f"{case} {tensor}: float32 reference {err_ref32:.3e} is at or above the cap {CAP}"
    elif accept(err_engine, err_ref32, floor):
        verdict, bad = "ok", None
    else:
        verdict = "FAIL"
        bad = f"{case} {tensor}: {who} {err_engine:.3e}, float32 reference {err_ref32:.3e}, floor {floor:.1e}"
    ROWS.row(case, tensor, who, err_engine, err_ref32, f"floor {floor:7.1e}", verdict)
    return bad


log_value = ROWS.write


def _d(t):
    return t.detach().to(device="cpu", dtype=torch.float64)


def worst_slice_err(a, ref64, dims):
    """max over the slices that `dims` sum over of the relative L2 of one slice"""
    a, b = _d(a), _d(ref64)
    den = (b * b).sum(dims).sqrt()
    return float((((a - b) ** 2).sum(dims).sqrt() / torch.where(den > 0, den, torch.ones_like(den))).max())


def max_over_rms(a, ref64):
    a, b = _d(a), _d(ref64)
    rms = float((b * b).mean().sqrt())
    return float((a - b).abs().max()) / (rms if rms > 0 else 1.0)


def scalar_err(a, ref):
    a, ref = float(a), float(ref)
    return abs(a - ref) / (abs(ref) if ref != 0 else 1.0)


def loss_f_of_field(field, f, dtype):
    """mean_b ||field_b|| / ||f repeated over T - 2|| with torch.norm in `dtype` on the CPU"""
    B, planes = field.shape[:2]
    x = field.detach().to(device="cpu", dtype=dtype).reshape(B, -1)
    y = f.to(dtype).reshape(1, 1, -1).repeat(B, planes, 1).reshape(B, -1)
    return torch.mean(torch.norm(x, 2, 1) / torch.norm(y, 2, 1))


def forward_failures(case, got, ref32, ref64, f, who="engine", floor_case=False):
    """got: {"loss_ic", "loss_f", "field"}"""
    kw = dict(who=who, log_only=floor_case)
    own64 = loss_f_of_field(got["field"], f, torch.float64)
    bad = [judge(case, "field", rel_err(got["field"], ref64["field"]), rel_err(ref32["field"], ref64["field"]), **kw),
           judge(case, "field/plane", worst_slice_err(got["field"], ref64["field"], (2, 3)),
                 worst_slice_err(ref32["field"], ref64["field"], (2, 3)), **kw),
           judge(case, "max|e|/rms", max_over_rms(got["field"], ref64["field"]), max_over_rms(ref32["field"], ref64["field"]), **kw),
           judge(case, "loss_f/own", scalar_err(got["loss_f"], own64),
                 scalar_err(loss_f_of_field(got["field"], f, torch.float32), own64), **kw),
           judge(case, "loss_f", scalar_err(got["loss_f"], ref64["loss_f"]), scalar_err(ref32["loss_f"], ref64["loss_f"]),
                 who=who, log_only=True),
           judge(case, "loss_ic", scalar_err(got["loss_ic"], ref64["loss_ic"]), scalar_err(ref32["loss_ic"], ref64["loss_ic"]), **kw)]
    return [b for b in bad if b]


def grad_failures(case, grad, ref32n, ref32, ref64, who="engine", floor_case=False):
    """dL/du overall and the worst time level (levels 0, 1, T - 2, T - 1 take different branches of k_pino_assemble), judged
    against the float32 oracle with float64 norms; the plain float32 oracle's error is logged"""
    kw = dict(who=who, log_only=floor_case)
    bad = [judge(case, "grad", rel_err(grad, ref64["grad"]), rel_err(ref32n["grad"], ref64["grad"]), **kw),
           judge(case, "grad/level", worst_slice_err(grad, ref64["grad"], (0, 1, 2)),
                 worst_slice_err(ref32n["grad"], ref64["grad"], (0, 1, 2)), **kw),
           judge(case, "grad:ref32", rel_err(grad, ref64["grad"]), rel_err(ref32["grad"], ref64["grad"]), who=who, log_only=True)]
    return [b for b in bad if b]
