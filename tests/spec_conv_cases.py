"""What the standalone spectral convolution (fno_spec_forward / fno_spec_backward, functional.spectral_conv and the
spectral branch of functional.spectral_pointwise_layer) is held to: the cases, three evaluations, the sliced comparison and the
error table.  Shared by tests/test_spec_conv_gpu.py (the HIP kernels, each case behind an assertion on the launch log) and
tests/test_spec_conv_reference.py (the float32 oracle alone, and planted faults that the slices must refuse).

Evaluations: ref64 = oracle/fno_oracle.py on float64 copies of the float32 inputs, ref32 = the same oracle in float32 on the
CPU, and the engine.  Criterion (tests/judging.py::accept, the numbers of DESIGN 4l / 4n) for every quantity:
    e_engine == 0 or e_engine < max(FLOOR, BUDGET_SLACK * e_ref32),   FLOOR = 2e-6,
both errors taken against ref64, a sliced quantity being the WORST slice of the engine against the WORST slice of ref32.
The whole-tensor line of tests/test_parity_gpu.py (relative L2 against ref32 under TOL_COMP = 5e-6) is judged beside it.

Quantities.  y (B, Cout, P.., W) and dx:
    whole    relative L2 over everything
    /row     worst (b, p): relative L2 over channels and W of one row of the flattened leading dims - one row in thousands
             that a partial row block got wrong is 1 / sqrt(rows) of the whole tensor and the whole of its own slice
    /chan    worst (b, c)
    /mode    worst kept mode: |rfftn(error)| over |rfftn(ref64)|, both over (b, c), at one bin of the kept set
    leak     norm of rfftn off the kept set over the norm on it (y only; dialect A: bias subtracted first)
    leak/bin worst single bin off the kept set over the rms bin on it.  The total above dilutes one leaking bin by
             sqrt(kept bins) exactly as the whole tensor dilutes one wrong mode; this one does not.
The kept set comes from the mode indices: rows [0, m) and [N - m, N) of every leading dim, bins [0, live) of the last one - and,
on the self-conjugate planes of the last dim (bin 0; bin W / 2 of an even W), their mirror images, since irfftn returns the real
signal whose half spectrum is the Hermitian part of what it was given (row N - m of bin 0 comes back in row m too).
dW per corner (Cin, Cout, m.., wl): whole, /mode (worst (Cin x Cout) slice of one stored mode), /cin, /cout.  Gradients that are
structurally zero - planes [live, wl) of dialect C in 3-D, the first corner's rows shadowed by an overlapping second corner - must
BE zero and are left out of the slices.  dbias: worst channel, |error| over rms(dy) sqrt(B PW) (the size of a sum of B PW terms).
Every row goes to the file $SPEC_CONV_ERROR_LOG names."""
import functools
import typing

import numpy as np
import torch
import torch.nn.functional as TF

from oracle import fno_oracle as O
from oracle.detfill import fill_named
from tests.judging import TOL_COMP, RowLog, accept, rel_err
from tests.step_tail_cases import FLOOR_GATE

FLOOR = FLOOR_GATE
ROWS = RowLog("SPEC_CONV_ERROR_LOG", widths=(26, 14))
NORM = {"A": "forward", "B": "ortho", "C": "backward"}


class Case(typing.NamedTuple):
    name: str
    dialect: str                 # A (bias, norm "forward"), B (square 2-D, "ortho"), C ("backward")
    B: int
    cin: int
    cout: int
    dims: tuple
    modes: tuple                 # extents of the stored corner weights; the live last extent is min(W // 2 + 1, modes[-1])
    gelu: bool = False           # through spectral_pointwise_layer(input_gelu=True) with a zero pointwise branch: y = conv(gelu(u))

    @property
    def live(self):
        return tuple(self.modes[:-1]) + (min(self.dims[-1] // 2 + 1, self.modes[-1]),)

    @property
    def P(self):
        return int(np.prod(self.dims[:-1]))

    @property
    def Ktot(self):
        return int(np.prod([2 * m for m in self.live[:-1]])) * self.live[-1]

    @property
    def id(self):
        return self.name.replace(" ", "_")


def _c(name, dialect, shape, modes, cout=None, gelu=False):
    return Case(name, dialect, shape[0], shape[1], cout or shape[1], tuple(shape[2:]), tuple(modes), gelu)


# Row passes: one case per route and edge of row_forward / row_inverse (fno_abi.hip), each the smallest that reaches it on
# 256 compute units (rows per workgroup shrink until B ceil(P / rb) >= 4 x 256 tiles; persistent grids hold <= 4 x 256).
ROW_CASES = [
    _c("rows rb2 partial", "C", (2, 34, 1025, 73), (5, 12)),
    _c("rows rb4 partial loop", "C", (2, 34, 45, 47, 73), (3, 4, 12)),
    _c("rows mfma rb4 partial", "C", (2, 32, 45, 47, 33), (3, 4, 12)),
    _c("rows rb1 loop 32", "C", (5, 32, 211, 33), (5, 12)),
    _c("rows rb1 loop 34", "C", (5, 34, 211, 73), (5, 12)),
    _c("chan4 q4 loop", "C", (3, 32, 16, 32, 73), (3, 4, 12)),
    _c("chan4 rb16 loop", "C", (18, 64, 128, 40), (3, 12)),
    _c("flat tile partial", "C", (2, 32, 24, 43, 41), (3, 4, 12)),
    _c("tile loop uneven", "B", (7, 32, 448, 32), (6, 9)),
    _c("gelu chan4", "C", (7, 32, 448, 32), (6, 9), gelu=True),
]
MULTI_ROW = ROW_CASES[:3]

# The contraction.  Stream kernels (k_mode_gemv<B>, k_mode_outer_dw<B>: B <= 4, <= 64 channels, Ktot Cin Cout >= 2^21) at
# Ktot = 34 x 21 = 714, Ktot % 4 = 2 against a grid of ceil(Ktot / 4), the leading extent 34 on k_axis_generic.  (17, 17) kept
# modes give Ktot Cin Cout = 578 x 48 x 64 = 1.78 M, under the threshold: that shape takes the batched kernels.)
STREAM_CASES = [_c(f"stream B{b}", "C", (b, 48, 64, 64), (17, 21), cout=64) for b in (3, 2, 4)]
# Cin != Cout: the LDS form (512 % Cout == 0) chunks the batch by bt = 2 (512 / Cout) and the input channels by it = bt; the plain
# form by nb = ni = 256 / Cout.  B = 9 is no multiple of either; 40 -> 64 leaves Cin % it = 8 (48 and 128 divide).
GEMM_CASES = [
    _c("gemm lds 48>64", "C", (9, 48, 8, 16), (3, 5), cout=64),
    _c("gemm lds 40>64", "C", (9, 40, 8, 16), (3, 5), cout=64),
    _c("gemm lds 128>128", "C", (9, 128, 8, 16), (3, 5)),
    _c("gemm plain 34>20", "C", (9, 34, 8, 16), (3, 5), cout=20),
    _c("gemm plain 64>96", "C", (9, 64, 8, 16), (3, 5), cout=96),
]
# Leading-axis passes at width 32: every template extent 2 m (from 24 on with the twiddle table in LDS), 14 on k_axis_generic;
# 34 channels x 5 bins = 170 complex columns, no multiple of 64.  Dialect B needs a square grid, C takes N = 2 m + 5.
AXIS_M = (2, 3, 4, 5, 6, 8, 12, 16, 20, 7)
AXIS_CASES = [_c(f"axis m{m} {'B' if i % 2 else 'C'}", "B" if i % 2 else "C",
                 (2, 34, 32 if i % 2 else 2 * m + 5, 32), (m, 5)) for i, m in enumerate(AXIS_M)]
AXIS_CASES += [
    _c("axis 3d dead planes", "C", (2, 34, 9, 11, 16), (2, 3, 12)),        # two leading dims; live last extent 9 of 12 stored
    _c("axis sweep 320", "C", (1, 32, 320, 32), (20, 5)),                   # 320 x 40 twiddles exceed the 96 KB table: generic
    _c("overlap A", "A", (2, 32, 8, 16), (6, 6)),                           # 2 m > N: rows 2..5 of corner 0 are shadowed
]
DBIAS_CASES = [_c("dbias scalar arm", "A", (2, 34, 9, 33), (3, 5))]         # PW = 297, PW % 4 = 1
ALL_CASES = ROW_CASES + STREAM_CASES + GEMM_CASES + AXIS_CASES + DBIAS_CASES
CASE = {c.name: c for c in ALL_CASES}
assert len(CASE) == len(ALL_CASES)
assert all(c.B * max(c.cin, c.cout) * int(np.prod(c.dims)) <= 11_000_000 for c in ALL_CASES)


# ---------------------------------------------------------------------------------------------------------------------
# inputs and the oracle
# ---------------------------------------------------------------------------------------------------------------------
def ncorner(case):
    return 2 ** (len(case.dims) - 1)


def make_inputs(case):
    """{"x", "dy", "w": [corner weights, real (Cin, Cout, m.., 2), in the ORACLE's order], "bias" (dialect A) or None}, float32"""
    tag = "sc." + case.name
    nd = len(case.dims)
    inp = {"x": torch.from_numpy(fill_named(tag + ".x", (case.B, case.cin) + case.dims, 1.0)),
           "dy": torch.from_numpy(fill_named(tag + ".dy", (case.B, case.cout) + case.dims, 1.0)),
           "w": [torch.from_numpy(fill_named(f"{tag}.w{i}", (case.cin, case.cout) + case.modes + (2,), 0.02))
                 for i in range(ncorner(case))],
           "bias": torch.from_numpy(fill_named(tag + ".bias", (case.cout,) + (1,) * nd, 0.1)) if case.dialect == "A" else None}
    return inp


def engine_order(case):
    """engine corner i is oracle corner engine_order[i]: (lo,lo), (lo,hi), (hi,lo), (hi,hi) against basics.py:127-134's
    w1 (lo,lo), w2 (hi,lo), w3 (lo,hi), w4"""
    return [0, 2, 1, 3] if (case.dialect == "C" and len(case.dims) == 3) else list(range(ncorner(case)))


def oracle_forward(case, x, wc, bias):
    if case.gelu:
        x = TF.gelu(x)
    if case.dialect == "B" and case.dims[0] != case.dims[1]:
        # rno.py:66-67 transforms to (n, n) with n the LAST extent: the reference's dialect B exists on square grids only.  Off
        # them, the same operator ("ortho", two corners, bins [0, m)) is dialect A's without bias.
        return O.spectral_conv_A(x, wc, None, list(case.modes), "ortho")
    if case.dialect == "B":
        return O.spectral_conv_B(x, torch.view_as_real(wc[0]), torch.view_as_real(wc[1]), *case.modes)
    if case.dialect == "C":
        return O.spectral_conv_C3d(x, *wc, *case.modes) if len(case.dims) == 3 else O.spectral_conv_C2d(x, *wc, *case.modes)
    return O.spectral_conv_A(x, wc, bias, list(case.modes), "forward")


def oracle_eval(case, inp, dtype, batch=None):
    """{"y", "dx", "dw": [complex per corner, oracle order], "dbias" (Cout,) or None} in `dtype` on copies of the inputs;
    batch: a slice of the samples (the weight gradient of part of the batch)"""
    sl = slice(None) if batch is None else batch
    x = inp["x"][sl].to(dtype).clone().requires_grad_(True)
    ws = [w.to(dtype).clone().requires_grad_(True) for w in inp["w"]]
    bias = inp["bias"].to(dtype).clone().requires_grad_(True) if inp["bias"] is not None else None
    y = oracle_forward(case, x, [torch.view_as_complex(w) for w in ws], bias)
    y.backward(inp["dy"][sl].to(dtype))
    return {"y": y.detach(), "dx": x.grad, "dw": [torch.view_as_complex(w.grad) for w in ws],
            "dbias": bias.grad.reshape(-1) if bias is not None else None}


@functools.lru_cache(maxsize=2)
def references(name):
    """(inputs, ref64, ref32) of one case, computed once and shared; nobody writes into them"""
    case = CASE[name]
    inp = make_inputs(case)
    return inp, oracle_eval(case, inp, torch.float64), oracle_eval(case, inp, torch.float32)


# ---------------------------------------------------------------------------------------------------------------------
# the kept set and the structural zeros, from the mode indices
# ---------------------------------------------------------------------------------------------------------------------
def kept_mask(case):
    """bool (d1.., W // 2 + 1): the bins of rfftn(y) the operator can fill"""
    W = case.dims[-1]
    mask = np.zeros(W // 2 + 1, bool)
    mask[:case.live[-1]] = True
    for n, m in zip(reversed(case.dims[:-1]), reversed(case.live[:-1])):
        lead = np.zeros(n, bool)
        lead[:m] = True
        lead[n - m:] = True
        mask = lead.reshape((n,) + (1,) * mask.ndim) & mask[None]
    mask = np.ascontiguousarray(mask)
    for k in {0, W // 2} if W % 2 == 0 else {0}:
        if k < case.live[-1]:
            plane = mask[..., k]
            mirror = plane
            for ax in range(plane.ndim):
                mirror = np.roll(np.flip(mirror, ax), 1, ax)
            mask[..., k] = plane | mirror
    return torch.from_numpy(mask)


def dw_live_mask(case, corner):
    """bool (m.., wl) over the stored modes of oracle corner `corner`: False where the gradient is structurally zero"""
    mask = np.ones(case.modes, bool)
    mask[..., case.live[-1]:] = False
    if len(case.dims) == 2 and corner == 0:
        n, m = case.dims[0], case.modes[0]
        mask[max(n - m, 0):m] = False                 # rows r < m with r >= N - m belong to the second corner
    return torch.from_numpy(mask)


# ---------------------------------------------------------------------------------------------------------------------
# the quantities
# ---------------------------------------------------------------------------------------------------------------------
def _d(t):
    return t.detach().to(device="cpu", dtype=torch.complex128 if t.is_complex() else torch.float64)


def _worst(num, den):
    """(max of sqrt(num / den) over the entries with den > 0, its flat index)"""
    r = torch.where(den > 0, num / torch.where(den > 0, den, torch.ones_like(den)), torch.zeros_like(den)).sqrt().reshape(-1)
    i = int(r.argmax())
    return float(r[i]), i


def _sq(t):
    return (t.real ** 2 + t.imag ** 2) if t.is_complex() else t * t


def field_errors(case, a, ref64, bias=None, leak=False):
    """{"whole", "/row", "/chan", "/mode" (, "leak", "leak/bin")} of a (B, C, dims) tensor; also "@row" etc.: where the worst is"""
    a, r = _d(a), _d(ref64)
    B, C = r.shape[:2]
    e2, r2 = ((a - r) ** 2).reshape(B, C, case.P, -1), (r * r).reshape(B, C, case.P, -1)
    out = {"whole": float(e2.sum().sqrt() / r2.sum().sqrt())}
    out["/row"], out["@row"] = _worst(e2.sum((1, 3)), r2.sum((1, 3)))
    out["/chan"], out["@chan"] = _worst(e2.sum((2, 3)), r2.sum((2, 3)))
    sp = tuple(range(2, r.dim()))
    mask = kept_mask(case)
    E, R = _sq(torch.fft.rfftn(a - r, dim=sp)).sum((0, 1)), _sq(torch.fft.rfftn(r, dim=sp)).sum((0, 1))
    out["/mode"], out["@mode"] = _worst(torch.where(mask, E, torch.zeros_like(E)), R)
    if leak:
        A = _sq(torch.fft.rfftn(a if bias is None else a - _d(bias).reshape(1, C, *([1] * len(sp))), dim=sp)).sum((0, 1))
        on, off = A[mask], A[~mask]
        out["leak"] = float(off.sum().sqrt() / on.sum().sqrt())
        out["leak/bin"] = float(off.max().sqrt() / on.mean().sqrt())
    return out


def dw_errors(case, corner, a, ref64):
    """{"whole", "/mode", "/cin", "/cout", "zeros": True when every structurally zero entry IS zero} of one corner gradient"""
    a, r = _d(a), _d(ref64)
    live = dw_live_mask(case, corner)
    e2, r2 = _sq(a - r) * live, _sq(r) * live
    md = tuple(range(2, r.dim()))
    out = {"whole": float(e2.sum().sqrt() / r2.sum().sqrt()), "zeros": bool((a[..., ~live] == 0).all())}
    out["/mode"], out["@mode"] = _worst(e2.sum((0, 1)), r2.sum((0, 1)))
    out["/cin"], out["@cin"] = _worst(e2.sum((1,) + md), r2.sum((1,) + md))
    out["/cout"], out["@cout"] = _worst(e2.sum((0,) + md), r2.sum((0,) + md))
    return out


def dbias_error(case, a, ref64, dy):
    scale = float(_d(dy).pow(2).mean().sqrt()) * (case.B * case.P * case.dims[-1]) ** 0.5
    return float((_d(a) - _d(ref64)).abs().max()) / scale


# ---------------------------------------------------------------------------------------------------------------------
# the comparison and the error table
# ---------------------------------------------------------------------------------------------------------------------
def judge(case, quantity, err, err_ref32, who="engine", floor=FLOOR, fixed=None):
    """One row of the table and a description of the failure, or None.  fixed: a plain bound instead of the budget."""
    ok = (err < fixed) if fixed is not None else accept(err, err_ref32, floor)
    ROWS.row(case, quantity, who, err, err_ref32, f"bound {fixed:7.1e}" if fixed is not None else f"floor {floor:7.1e}",
             "ok" if ok else "FAIL")
    return None if ok else f"{case} [{quantity}] {who} {err:.3e}, float32 reference {err_ref32:.3e}, " + \
        (f"bound {fixed:.1e}" if fixed is not None else f"floor {floor:.1e}")


def quantities(case, got, ref64, inp, only=("y", "dx", "dw", "dbias")):
    """{quantity name: error against ref64} of one evaluation (got: {"y", "dx", "dw", "dbias"} like the references; tensors not
    in `only` are not read), and the list of corner gradients whose structurally zero entries are not zero"""
    q, nonzero = {}, []
    for t in ("y", "dx"):
        if t in only:
            leak = t == "y" and not case.gelu        # (the layer's dx carries gelu'(u): not band-limited)
            e = field_errors(case, got[t], ref64[t], inp["bias"] if leak else None, leak)
            q.update({t + ("" if k == "whole" else k if k[0] == "/" else ":" + k): v for k, v in e.items() if k[0] != "@"})
    if "dw" in only:
        for c in range(ncorner(case)):
            e = dw_errors(case, c, got["dw"][c], ref64["dw"][c])
            q.update({f"dw{c}" + ("" if k == "whole" else k): v for k, v in e.items() if k[0] == "/" or k == "whole"})
            if not e["zeros"]:
                nonzero.append(f"dw{c}")
    if "dbias" in only and ref64["dbias"] is not None:
        q["dbias/chan"] = dbias_error(case, got["dbias"], ref64["dbias"], inp["dy"])
    return q, nonzero


def failures(case, got, ref32, ref64, inp, who="engine", only=("y", "dx", "dw", "dbias")):
    """every judged row of one case as "case [quantity] ..." descriptions of what failed"""
    (g, nonzero), (r, _) = quantities(case, got, ref64, inp, only), quantities(case, ref32, ref64, inp, only)
    bad = [judge(case.name, k, g[k], r[k], who) for k in g]
    bad += [f"{case.name} [{k}:zeros] a structurally zero gradient is not zero" for k in nonzero]
    whole = [t for t in ("y", "dx") if t in only] + ([f"dw{c}" for c in range(ncorner(case))] if "dw" in only else [])
    for t in whole:
        a, b = (v["dw"][int(t[2:])] if t[:2] == "dw" else v[t] for v in (got, ref32))
        if a.is_complex():
            a, b = torch.view_as_real(a), torch.view_as_real(b)
        bad.append(judge(case.name, t + ":TOL_COMP", rel_err(a, b), 0.0, who, fixed=TOL_COMP))
    return [b for b in bad if b]


def blamed(bad):
    """the quantities a list of failures names"""
    return {b[b.index("[") + 1:b.index("]")] for b in bad}
