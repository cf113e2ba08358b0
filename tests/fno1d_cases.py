"""Cases, inputs, float64 / float32 references and the judged quantities of the one-dimensional spectral convolution
(csrc/k_spec1d.h) and the two FNO1d models built on it.  Float64 truth is torch on the CPU: dialect A and the neuralop model
through oracle.fno_oracle (spectral_conv_A / fno_forward, order-generic), dialect C and the PINO model through the few lines of
torch.fft below, which restate libs/models/pino_models/basics.py:47-58 and fourier1d.py:45-62 of the reference.

Criterion (tests.judging.judge_budget): err == 0 or err < max(1e-5, 1.75 x the float32 torch evaluation's own distance from
float64).  A CPU emulation of the kernels' summation order (fp32 tables, sequential fp32 accumulation over 256-point slabs) sits
2.5e-7 .. 4.9e-7 from float64 and the float32 FFT 1.5e-7 .. 2.1e-7, so the 1e-5 floor is the operative bound with ~20 x room.
Every achieved error is written to profiles/r19_fno1d_errors.txt before anything is asserted."""
import collections
import functools
import os

import torch
import torch.nn.functional as TF

from oracle import fno_oracle as O
from oracle.detfill import fill_named
from tests.judging import SectionLog, rel_err

LOG = SectionLog(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r19_fno1d_errors.txt"))
FLOOR = 1e-5

Case = collections.namedtuple("Case", "name dialect B cin cout N M norm bias wle")
CASES = [
    Case("A_one_tile", "A", 2, 32, 32, 128, 8, "forward", True, None),        # a single slab, nothing to reduce
    Case("C_three_tiles", "C", 3, 32, 64, 384, 16, "backward", False, None),   # unequal channels, N no power of two, partials to sum
    Case("A_max_modes", "A", 2, 64, 64, 256, 64, "ortho", True, None),        # widest accumulator, M at both limits
    Case("A_dc_only", "A", 2, 32, 32, 128, 1, "forward", True, None),         # the gamma = 1 bin alone
    Case("A_strided_w", "A", 2, 32, 32, 256, 12, "forward", True, 24),        # weight / gradient stride, dead half of dw untouched
    Case("A_long_row", "A", 1, 32, 32, 8192, 32, "forward", True, None),      # most slabs per sample, table at its largest
    # beyond the issue's table: a batch that is no multiple of the mix kernels' chunks - three chunks of 8 with a tail of 3 and
    # accumulators carried across them in k_s1_mix_bwd, a second grid row with a tail of 3 in k_s1_mix_fwd (the packed weights
    # written by row 0 only), dbias summed over 19 x 1 slab rows
    Case("A_batch_chunks", "A", 19, 32, 32, 256, 6, "forward", True, None),
]
CASE = {c.name: c for c in CASES}
LAYER = Case("layer_gelu", "A", 2, 64, 64, 256, 16, "forward", True, None)


def _t(name, shape, scale, complex_=False):
    return torch.from_numpy(fill_named("fno1d." + name, shape, scale, complex_=complex_))


def spectral_conv_C1d(x, w, modes1):
    """basics.py:47-58: rfft along the grid, the first modes1 bins times weights1 ("bix,iox->box", :10), zero elsewhere, irfft
    back to the input length; torch's default norm"""
    xf = torch.fft.rfft(x, dim=2)
    out = torch.zeros(x.shape[0], w.shape[1], x.shape[-1] // 2 + 1, dtype=xf.dtype)
    out[:, :, :modes1] = torch.einsum("bix,iox->box", xf[:, :, :modes1], w)
    return torch.fft.irfft(out, n=x.shape[-1], dim=2)


def conv_ref(case, x, w, bias):
    """the case's convolution on CPU tensors of one dtype; w complex (cin, cout, M)"""
    if case.dialect == "C":
        return spectral_conv_C1d(x, w, case.M)
    return O.spectral_conv_A(x, [w], None if bias is None else bias.reshape(-1, 1), [case.M], case.norm)


@functools.lru_cache(maxsize=None)
def inputs(name):
    c = CASE[name] if name in CASE else LAYER
    wl = c.wle or c.M
    inp = {"x": _t(name + ".x", (c.B, c.cin, c.N), 1.0), "dy": _t(name + ".dy", (c.B, c.cout, c.N), 1.0),
           "w": _t(name + ".w", (c.cin, c.cout, wl), 1.0 / c.cin, complex_=True),
           "bias": _t(name + ".bias", (c.cout,), 0.1) if c.bias else None}
    if c is LAYER:
        inp["pw"] = _t(name + ".pw", (c.cin, c.cin, 1), 1.0 / c.cin ** 0.5)
    return inp


def _grads(fn, tensors, dy, dtype):
    """(y, gradients in the order of `tensors`) of fn on copies of the given dtype (complex tensors: the matching complex one)"""
    cd = torch.complex128 if dtype == torch.float64 else torch.complex64
    ts = [None if t is None else t.detach().to(cd if t.is_complex() else dtype, copy=True).requires_grad_(True) for t in tensors]
    y = fn(*ts)
    live = [t for t in ts if t is not None]
    gs = iter(torch.autograd.grad(y, live, dy.to(dtype)))
    return y.detach(), [None if t is None else next(gs) for t in ts]


@functools.lru_cache(maxsize=None)
def references(name):
    """{dtype: {"y", "dx", "dw" (complex, the M live bins), "dbias"}} for float64 and float32, computed once and shared"""
    c, inp = CASE[name], inputs(name)
    out = {}
    for dt in (torch.float64, torch.float32):
        y, (dx, dw, db) = _grads(lambda x, w, b: conv_ref(c, x, w[..., :c.M], b), [inp["x"], inp["w"], inp["bias"]], inp["dy"], dt)
        out[dt] = {"y": y, "dx": dx, "dw": dw[..., :c.M], "dbias": db}
    return out


def layer_ref(x, w, pw, b, gelu, case=LAYER):
    a = TF.gelu(x) if gelu else x
    return O.spectral_conv_A(a, [w], None, [case.M], case.norm) + O.conv1x1(a, pw, b)


@functools.lru_cache(maxsize=None)
def layer_references(gelu):
    inp = inputs(LAYER.name)
    out = {}
    for dt in (torch.float64, torch.float32):
        y, (du, dw, dpw, db) = _grads(lambda x, w, pw, b: layer_ref(x, w, pw, b, gelu),
                                      [inp["x"], inp["w"], inp["pw"], inp["bias"]], inp["dy"], dt)
        out[dt] = {"y": y, "du": du, "dw": dw, "dpw": dpw, "dbias": db}
    return out


def worst_mode(dw, ref64):
    """the largest relative error of one kept bin of a weight gradient (cin, cout, M)"""
    return max(rel_err(torch.view_as_real(dw[..., k]), torch.view_as_real(ref64[..., k])) for k in range(ref64.shape[-1]))


def rows(got, ref):
    """judge_budget rows for every quantity of `got` (name -> tensor) against ref[float64] / ref[float32]; complex weight
    gradients also by their worst kept bin"""
    out = []
    r64, r32 = ref[torch.float64], ref[torch.float32]
    for k, v in got.items():
        if v is None:
            continue
        re = (lambda t: torch.view_as_real(t.resolve_conj())) if v.is_complex() else (lambda t: t)
        out.append((k, rel_err(re(v), re(r64[k])), rel_err(re(r32[k]), re(r64[k])), FLOOR))
        if v.is_complex():
            out.append((k + " worst bin", worst_mode(v, r64[k]), worst_mode(r32[k], r64[k]), FLOOR))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the models
# ---------------------------------------------------------------------------------------------------------------------
def neuralop_params(model, tag):
    """deterministic values for every parameter of a neuralop FNO1d (name -> float32 tensor of the parameter's shape)"""
    p = {}
    for n, v in model.state_dict().items():
        fan = v.shape[1] if v.dim() > 1 and "convs" not in n else 1
        scale = 1.0 / v.shape[0] if "convs.weight" in n else (0.1 if v.dim() == 1 or "bias" in n else 1.0 / fan ** 0.5)
        p[n] = _t(f"{tag}.{n}", tuple(v.shape), scale)
    return p


def pino_fno1d_forward(p, x, modes, act):
    """fourier1d.py:45-62: fc0, (B, N, C) -> (B, C, N), per layer SpectralConv1d + Conv1d(k=1) with the activation between
    layers (not behind the last), back to (B, N, C), fc1, activation, fc2"""
    f = {"gelu": TF.gelu, "relu": TF.relu}[act]
    h = (x @ p["fc0.weight"].T + p["fc0.bias"]).permute(0, 2, 1)
    for i, m in enumerate(modes):
        h = spectral_conv_C1d(h, p[f"sp_convs.{i}.weights1"], m) + O.conv1x1(h, p[f"ws.{i}.weight"], p[f"ws.{i}.bias"])
        if i != len(modes) - 1:
            h = f(h)
    h = f(h.permute(0, 2, 1) @ p["fc1.weight"].T + p["fc1.bias"])
    return h @ p["fc2.weight"].T + p["fc2.bias"]


def pino_params(model, tag):
    p = {}
    for n, v in model.state_dict().items():
        if v.is_complex():
            p[n] = _t(f"{tag}.{n}", tuple(v.shape), 1.0 / v.shape[0], complex_=True)
        else:
            p[n] = _t(f"{tag}.{n}", tuple(v.shape), 0.1 if v.dim() == 1 else 1.0 / v.shape[1] ** 0.5)
    return p


def model_reference(forward, p, x, dy):
    """{dtype: {"y", "grad <name>"}} of forward(params, x) for float64 and float32"""
    out = {}
    names = list(p)
    for dt in (torch.float64, torch.float32):
        y, gs = _grads(lambda *ts: forward(dict(zip(names, ts[:-1])), ts[-1]), [p[n] for n in names] + [x], dy, dt)
        out[dt] = {"y": y, **{"grad " + n: g for n, g in zip(names, gs[:-1])}}
    return out
