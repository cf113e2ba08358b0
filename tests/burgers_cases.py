"""What the Burgers residual loss (csrc/k_burgers_loss.h, functional.burgers_loss / burgers_residual) and the model trained
with it (libs/models/pino_models/fourier2d.py, libs/pino_utils/train_2d.py) are held to: a helper module, not a conftest.

The loss.  `restated` states FDM_Burgers + PINO_loss (libs/pino_utils/losses.py:200-243 of the reference) and the EXPLICIT
adjoint in one dtype; in float64 it is the truth, in float32 the yardstick.  It takes the place of an oracle module: the
reference itself cannot run PINO_loss backward in float64 (its float32 `zeros` target breaks mse_loss).  The golden file
tests/golden/burgers_loss_small.npz holds the reference's own float32 results and ties the restatement to it
(tests/test_burgers_loss_host.py).

    dt = 1 / (nt - 1);  ux = D1 u, uxx = D2 u along x
    Du[b, j] = (u[b, j+1] - u[b, j-1]) / (2 dt) + ux[b, j] u[b, j] - visc uxx[b, j],   j = 1 .. nt-2
    loss_f = mean Du^2,  loss_u = mean (u[:, 0] - u0)^2
    r = g_f 2 Du / (B (nt-2) nx)  (0 on rows 0 and nt-1)
    du = r ux - D1(r u) - visc D2 r;  du[j+1] += r[j] / (2 dt), du[j-1] -= r[j] / (2 dt);  du[:, 0] += g_u 2 (u[:, 0] - u0) / (B nx)

D1 / D2 are the real circulant operators of irfft(m(k) fft(u)[: nx/2 + 1]): m1 = 2 pi i k without the Nyquist bin (irfft
drops its purely imaginary coefficient), m2 = -(2 pi k)^2 with it.

Input families, built in float64 from oracle.detfill and rounded once: white (uniform +-1) and smooth (five Fourier modes in x
with amplitudes 1 / m, drifting and decaying in t); u0 = u[:, 0] + 0.1 fill.

Criterion: tests.judging.judge_budget (slack 1.75), floor FLOOR_GATE = 2e-6 for fields, losses and du; a float32 yardstick
at or above CAP = 0.1 is a failure by itself, so no row is ever left out.  Every figure goes to
profiles/r20_burgers_errors.txt before anything is asserted."""
import functools
import math
import os

import numpy as np
import torch
import torch.nn.functional as TF

from oracle import fno_oracle as O
from oracle.detfill import fill_named, name_seed, unit_fill
from tests.judging import SectionLog, rel_err
from tests.step_tail_cases import FLOOR_GATE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
LOG = SectionLog(os.path.join(ROOT, "profiles", "r20_burgers_errors.txt"))
FLOOR = FLOOR_GATE
FLOOR_BIAS = 2e-5                            # bias sums of the model (the channel-MLP floors)
CAP = 0.1
IC_WEIGHT = 5.0
TJ = 8                                       # csrc/k_burgers_loss.h BURG_TJ: interior rows per workgroup
VISCS = (0.01, 0.1)
# (B, nt, nx): one interior row; the golden small case; the golden case; two tiles + halo at nx 64; the workload's grid;
# nt - 2 = TJ (one full tile, no partner tile) and nt - 2 = 2 TJ + 1 (a third tile of one row, its pair partner absent)
SHAPES = ((1, 3, 32), (2, 5, 32), (3, 11, 128), (2, 34, 64), (2, 101, 128), (2, TJ + 2, 64), (2, 2 * TJ + 3, 64))
GOLDEN_CASES = (("white", (2, 5, 32)), ("white", (3, 11, 128)), ("smooth", (3, 11, 128)))
GOLDEN_VISC = 0.01


def families(shape):
    return ("white", "smooth") if shape[1] >= 11 else ("white",)


def case_name(family, shape, visc):
    return f"burgers {family} B={shape[0]} nt={shape[1]} nx={shape[2]} visc={visc:g}"


@functools.lru_cache(maxsize=None)
def make_inputs(family, shape):
    """{"u" (B, nt, nx), "u0" (B, nx)} float32 on the CPU"""
    B, nt, nx = shape
    tag = f"burgers.{family}.{B}.{nt}.{nx}"
    if family == "white":
        u = fill_named(tag + ".u", (B, nt, nx), 1.0, dtype=np.float64)
    elif family == "smooth":
        t = (np.arange(nt, dtype=np.float64) / (nt - 1))[None, :, None]
        x = (np.arange(nx, dtype=np.float64) / nx)[None, None, :]
        u = np.zeros((B, nt, nx))
        for m in range(1, 6):
            phase = math.pi * unit_fill((B,), name_seed(f"{tag}.phase.{m}"))[:, None, None]
            speed = 0.3 + 0.2 * unit_fill((B,), name_seed(f"{tag}.speed.{m}"))[:, None, None]
            u += (1.0 / m) * np.exp(-0.3 * m * t) * np.sin(2.0 * math.pi * m * (x - speed * t) + phase)
    else:
        raise ValueError(family)
    u0 = u[:, 0] + 0.1 * fill_named(tag + ".u0", (B, nx), 1.0, dtype=np.float64)
    return {"u": torch.from_numpy(u.astype(np.float32)), "u0": torch.from_numpy(u0.astype(np.float32))}


# ---------------------------------------------------------------------------------------------------------------------
# the restatement, one dtype throughout, with the explicit adjoint
# ---------------------------------------------------------------------------------------------------------------------
FAULTS = ("nyquist_d1", "adjoint_sign", "dt_slip", "mean_rows", "tile_edge")


def _multipliers(nx, dtype):
    k = torch.arange(nx // 2 + 1, dtype=dtype)
    a = 2.0 * math.pi * k
    a1 = a.clone()
    a1[-1] = 0.0
    return a1, -(a * a)


def d1(v):
    """the real circulant first derivative along the last dimension"""
    a1, _ = _multipliers(v.shape[-1], v.dtype)
    return torch.fft.irfft(1j * a1 * torch.fft.rfft(v, dim=-1), n=v.shape[-1], dim=-1)


def d2(v):
    _, m2 = _multipliers(v.shape[-1], v.dtype)
    return torch.fft.irfft(m2 * torch.fft.rfft(v, dim=-1), n=v.shape[-1], dim=-1)


def d1_nyquist_kept(v):
    """FAULT nyquist_d1.  Two real rows a, b travel as one complex line a + i b through a full complex transform (as the
    kernel packs them, the interior rows 1, 2 | 3, 4 | ..); with the table's Nyquist entry -nx/2 left in the multiplier the
    coefficient 2 pi i (-nx/2) (a_h + i b_h)[nx/2] is no longer purely imaginary, and row a takes pi nx b_h[nx/2] cos(pi nx x)
    from its partner (row b the opposite)."""
    B, rows, nx = v.shape
    k = torch.cat((torch.arange(0, nx // 2), torch.arange(-(nx // 2), 0))).to(v.dtype)
    out = torch.empty_like(v)
    inner = v[:, 1:rows - 1]
    if inner.shape[1] % 2:
        inner = torch.cat((inner, torch.zeros_like(inner[:, :1])), 1)
    z = torch.fft.ifft(2j * math.pi * k * torch.fft.fft(torch.complex(inner[:, 0::2], inner[:, 1::2]), dim=-1), dim=-1)
    both = torch.stack((z.real, z.imag), 2).reshape(B, -1, nx)
    out[:, 1:rows - 1] = both[:, :rows - 2]
    out[:, 0], out[:, rows - 1] = d1(v[:, 0]), d1(v[:, rows - 1])
    return out


def restated(u, u0, visc, dtype, g_u=IC_WEIGHT, g_f=1.0, fault=None):
    """{"loss_u", "loss_f" (0-dim), "field" (B, nt-2, nx), "grad" (B, nt, nx) = d(g_u loss_u + g_f loss_f)/du,
    "grad_f": the loss_f part alone}, everything in `dtype` on the CPU"""
    assert fault is None or fault in FAULTS
    u, u0 = u.to(dtype), u0.to(dtype)
    B, nt, nx = u.shape
    assert nx % 2 == 0
    dt = 1.0 / nt if fault == "dt_slip" else 1.0 / (nt - 1)
    rows = nt if fault == "mean_rows" else nt - 2
    ux = (d1_nyquist_kept if fault == "nyquist_d1" else d1)(u)
    uxx = d2(u)
    ut = (u[:, 2:] - u[:, :-2]) / (2 * dt)
    Du = ut + (ux * u - visc * uxx)[:, 1:-1]
    loss_f = (Du * Du).sum() / (B * rows * nx)
    d0 = u[:, 0] - u0
    loss_u = (d0 * d0).sum() / (B * nx)
    r = torch.zeros_like(u)
    r[:, 1:-1] = g_f * 2.0 * Du / (B * rows * nx)
    sign = 1.0 if fault == "adjoint_sign" else -1.0
    gf = r * ux + sign * d1(r * u) - visc * d2(r)
    up, down = r[:, :-1] / (2 * dt), r[:, 1:] / (2 * dt)          # r[j] into du[j+1], r[j] out of du[j-1]
    if fault == "tile_edge":                                     # rows j = 4 and 5 exchange nothing
        up, down = up.clone(), down.clone()
        up[:, 4] = 0.0                                           # r[4] does not reach du[5]
        down[:, 4] = 0.0                                         # r[5] does not reach du[4]
    gf[:, 1:] += up
    gf[:, :-1] -= down
    grad = gf.clone()
    grad[:, 0] += g_u * 2.0 * d0 / (B * nx)
    return {"loss_u": loss_u, "loss_f": loss_f, "field": Du, "grad": grad, "grad_f": gf}


@functools.lru_cache(maxsize=8)
def references(family, shape, visc, g_u=IC_WEIGHT, g_f=1.0):
    """(inputs, ref64, ref32) of one case, computed once and shared; nobody writes into them"""
    inp = make_inputs(family, shape)
    return (inp, restated(inp["u"], inp["u0"], visc, torch.float64, g_u, g_f),
            restated(inp["u"], inp["u0"], visc, torch.float32, g_u, g_f))


# ---------------------------------------------------------------------------------------------------------------------
# the judged quantities
# ---------------------------------------------------------------------------------------------------------------------
def _d(t):
    return t.detach().to(device="cpu", dtype=torch.float64)


def worst_row_err(a, ref64):
    """the largest relative L2 of one time row (over samples and x)"""
    a, b = _d(a), _d(ref64)
    den = (b * b).sum((0, 2)).sqrt()
    return float((((a - b) ** 2).sum((0, 2)).sqrt() / torch.where(den > 0, den, torch.ones_like(den))).max())


def scalar_err(a, ref):
    a, ref = float(a), float(ref)
    return abs(a - ref) / (abs(ref) if ref != 0 else 1.0)


def low_bins(t, bins=16):
    """projection onto the first `bins` bins in x"""
    h = torch.fft.rfft(_d(t), dim=-1)
    h[..., bins:] = 0
    return torch.fft.irfft(h, n=t.shape[-1], dim=-1)


def loss_rows(got, ref64, ref32):
    """judge_budget rows (name, err, err_ref32, floor) of got = {"loss_u", "loss_f", "field", "grad"} against the float64
    restatement, the float32 one as the yardstick.  loss_f is also held against the float64 mean of the engine's OWN stored
    field (the reduction alone; yardstick: the float32 mean of that field)."""
    own = _d(got["field"])
    own64 = float((own * own).mean())
    own32 = float((got["field"].detach().cpu().float() ** 2).mean())
    nt = ref64["grad"].shape[1]
    rows = [("field", rel_err(got["field"], ref64["field"]), rel_err(ref32["field"], ref64["field"]), FLOOR),
            ("field worst row", worst_row_err(got["field"], ref64["field"]), worst_row_err(ref32["field"], ref64["field"]), FLOOR),
            ("loss_f vs own field", scalar_err(got["loss_f"], own64), scalar_err(own32, own64), FLOOR),
            ("loss_f", scalar_err(got["loss_f"], ref64["loss_f"]), scalar_err(ref32["loss_f"], ref64["loss_f"]), FLOOR),
            ("loss_u", scalar_err(got["loss_u"], ref64["loss_u"]), scalar_err(ref32["loss_u"], ref64["loss_u"]), FLOOR)]
    if "grad" in got:
        rows += [("du", rel_err(got["grad"], ref64["grad"]), rel_err(ref32["grad"], ref64["grad"]), FLOOR),
                 ("du worst row", worst_row_err(got["grad"], ref64["grad"]), worst_row_err(ref32["grad"], ref64["grad"]), FLOOR)]
        for name, j in (("du row 0", 0), (f"du row nt-1", nt - 1)):
            rows.append((name, rel_err(got["grad"][:, j], ref64["grad"][:, j]), rel_err(ref32["grad"][:, j], ref64["grad"][:, j]),
                         FLOOR))
    capped = [name for name, _, ref, _ in rows if not ref < CAP]
    assert not capped, f"float32 yardstick at or above {CAP}: {capped}"
    return rows


# ---------------------------------------------------------------------------------------------------------------------
# the model: fourier2d.py:53-87 restated on oracle.fno_oracle's pieces, and the training loop around it
# ---------------------------------------------------------------------------------------------------------------------
MODES1, MODES2 = (4, 4, 3), (6, 6, 5)
MODEL_X = (2, 12, 32, 3)
GOLDEN_CIN = 8          # the golden file keeps a spectral weight's gradient for its first 8 input channels (file size)
MODEL_CASES = {"pad0": dict(pad_ratio=[0., 0.]), "pad_right": dict(pad_ratio=[0., 0.125])}
TRAIN_CFG = {"train": {"xy_loss": 1.0, "f_loss": 1.0, "ic_loss": 5.0, "epochs": 3, "save_dir": "burgers_test", "save_name": "t.pt"}}
TRAIN_VISC, TRAIN_LR = 0.01, 1e-3


def pads_of(pad_ratio, size_1, size_2):
    if max(pad_ratio) > 0:
        return [round(i * size_1) for i in pad_ratio], [round(i * size_2) for i in pad_ratio]
    return [0, 0], [0, 0]


def fno2d_forward(p, x, modes1, modes2, pad_ratio, act="gelu"):
    """p: name -> tensor (spectral weights complex); x (B, X, Y, in_dim)"""
    f = {"gelu": TF.gelu, "relu": TF.relu}[act]
    p1, p2 = pads_of(pad_ratio, x.shape[1], x.shape[2])
    h = (x @ p["fc0.weight"].T + p["fc0.bias"]).permute(0, 3, 1, 2)
    if max(p1) > 0 or max(p2) > 0:
        h = TF.pad(h, (p2[0], p2[1], p1[0], p1[1]), "constant", 0.)
    n = len(modes1)
    for i in range(n):
        h = (O.spectral_conv_C2d(h, p[f"sp_convs.{i}.weights1"], p[f"sp_convs.{i}.weights2"], modes1[i], modes2[i])
             + O.conv1x1(h, p[f"ws.{i}.weight"], p[f"ws.{i}.bias"]))
        if i != n - 1:
            h = f(h)
    if max(p1) > 0 or max(p2) > 0:
        h = h[..., p1[0]:-p1[1], p2[0]:-p2[1]]
    h = h.permute(0, 2, 3, 1)
    h = f(h @ p["fc1.weight"].T + p["fc1.bias"])
    h = f(h @ p["fc2.weight"].T + p["fc2.bias"])
    return h @ p["fc3.weight"].T + p["fc3.bias"]


def golden_params(g):
    """name -> float32 / complex64 tensor rebuilt from the golden file's fill scales and shapes"""
    p = {}
    for key in g.files:
        if not key.startswith("shapes/"):
            continue
        name = key[len("shapes/"):]
        shape, scale = tuple(int(s) for s in g[key]), float(g["scales/" + name])
        cplx = "weights" in name and "sp_convs" in name
        p[name] = torch.from_numpy(np.asarray(fill_named(name, shape, scale, complex_=cplx)))
    return p


def model_input(tag):
    return torch.from_numpy(fill_named("input:" + tag + ".x", MODEL_X, 1.0))


def to_dtype(p, dtype):
    cd = torch.complex128 if dtype == torch.float64 else torch.complex64
    return {k: v.detach().to(cd if v.is_complex() else dtype).clone() for k, v in p.items()}


def model_reference(p, x, modes1, modes2, pad_ratio, act, dtype):
    """{"y", "grad <name>"} of y.square().sum() in `dtype`"""
    q = {k: v.requires_grad_(True) for k, v in to_dtype(p, dtype).items()}
    y = fno2d_forward(q, x.to(dtype), modes1, modes2, pad_ratio, act)
    gs = torch.autograd.grad(y.square().sum(), list(q.values()))
    return {"y": y.detach(), **{"grad " + k: g for k, g in zip(q, gs)}}


def model_rows(got, ref64, ref32):
    """got / ref32: name -> tensor (complex or real (.., 2) spectral gradients both taken); bias sums get FLOOR_BIAS"""
    def re(t):
        t = t.detach().cpu()
        return torch.view_as_real(t.resolve_conj()) if t.is_complex() else t
    rows = []
    for k, v in ref64.items():
        floor = FLOOR_BIAS if k.endswith("bias") else FLOOR
        a, b32, b64 = re(got[k]), re(ref32[k]), re(v)
        rows.append((k, rel_err(a.reshape(b64.shape), b64), rel_err(b32.reshape(b64.shape), b64), floor))
    capped = [name for name, _, ref, _ in rows if not ref < CAP]
    assert not capped, f"float32 yardstick at or above {CAP}: {capped}"
    return rows


def train_data(tag="burgers_train"):
    """one batch of 2: x (2, 12, 32, 3) with x[:, 0, :, 0] the initial condition, y (2, 12, 32)"""
    x = model_input(tag)
    y = torch.from_numpy(fill_named("input:" + tag + ".y", MODEL_X[:3], 1.0))
    return x, y


def restated_training(p, x, y, modes1, modes2, pad_ratio, dtype, epochs=3, lr=TRAIN_LR, visc=TRAIN_VISC, cfg=TRAIN_CFG):
    """train_2d_burger (train_2d.py:119-194) on the restatements in `dtype`: one batch per epoch, torch.optim.Adam.
    Returns [(train_loss, train_pino, data_l2)]."""
    q = {k: v.requires_grad_(True) for k, v in to_dtype(p, dtype).items()}
    opt = torch.optim.Adam(list(q.values()), lr=lr)
    x, y = x.to(dtype), y.to(dtype)
    w = cfg["train"]
    hist = []
    for _ in range(epochs):
        out = fno2d_forward(q, x, modes1, modes2, pad_ratio).reshape(y.shape)
        B = y.shape[0]
        data = ((out - y).reshape(B, -1).norm(dim=1) / y.reshape(B, -1).norm(dim=1)).mean()
        B, nt, nx = out.shape
        Du = (out[:, 2:] - out[:, :-2]) / (2.0 / (nt - 1)) + (d1(out) * out - visc * d2(out))[:, 1:-1]
        loss_f = (Du * Du).mean()
        loss_u = ((out[:, 0] - x[:, 0, :, 0]) ** 2).mean()
        total = loss_u * w["ic_loss"] + loss_f * w["f_loss"] + data * w["xy_loss"]
        opt.zero_grad()
        total.backward()
        opt.step()
        hist.append((float(total.detach()), float(loss_f.detach()), float(data.detach())))
    return hist
