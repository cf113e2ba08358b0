"""What the Darcy residual loss (csrc/k_darcy_loss.h, functional.darcy_loss / darcy_residual) and the loops built on it
(libs/pino_utils/train_2d.py train_2d_operator, eval_2d.py) are held to: a helper module, not a conftest.

The loss.  `restated` states FDM_Darcy + darcy_loss (libs/pino_utils/losses.py:6-65 of the reference) with the mollifier and
the relative-L2 data term of the training loop, and the EXPLICIT adjoint, in one dtype; in float64 it is the truth, in float32
the yardstick.  tests/golden/darcy_loss_small.npz holds the reference's own float32 results and ties the restatement to it
(tests/test_darcy_loss_host.py).

    h = 1 / (S - 1);  pred = out * mol
    Du[b, p, q] = -( a[p+1,q] (pred[p+2,q] - pred[p,q]) - a[p-1,q] (pred[p,q] - pred[p-2,q])
                   + a[p,q+1] (pred[p,q+2] - pred[p,q]) - a[p,q-1] (pred[p,q] - pred[p,q-2]) ) / (4 h^2),   p, q = 2 .. S-3
    loss_f = mean_b ||Du_b - 1|| / (S - 4),  loss_data = mean_b ||pred_b - y_b|| / ||y_b||
    r = g_f (Du - 1) / (B (S-4) ||Du_b - 1||)  (0 off the residual cells; 0 for a sample whose norm is exactly zero)
    dpred[m,n] = -( a[m-1,n] r[m-2,n] + a[m+1,n] r[m+2,n] - (a[m+1,n] + a[m-1,n]) r[m,n]
                  + a[m,n-1] r[m,n-2] + a[m,n+1] r[m,n+2] - (a[m,n+1] + a[m,n-1]) r[m,n] ) / (4 h^2)
                 + g_data (pred - y)[m,n] / (B ||pred_b - y_b|| ||y_b||),   dout = mol * dpred

Input families, built in float64 from oracle.detfill and rounded once:
  white  out uniform +-1, a uniform in [0.5, 2]
  darcy  a is 12 where a nine-mode cosine field is positive and 3 elsewhere; out = 8 + 3 g with g nine sine modes of amplitude
         1 / (m n), so that with the training mollifier 0.001 sin(pi x) sin(pi y) Du - 1 is O(1), as in training
`mol` is the training mollifier built as train_2d.py builds it; `u` is the float32 product out * mol for darcy and `out` for
white: what a case without the mollifier takes as the model output.  y = u + 0.1 rms(u) fill.

Criterion: tests.judging.judge_budget (slack 1.75), floor FLOOR_GATE = 2e-6; a float32 yardstick at or above CAP = 0.1 is a
failure by itself, so no row is ever left out.  Every figure goes to profiles/r21_darcy_errors.txt before anything is asserted."""
import functools
import math
import os

import numpy as np
import torch

from oracle.detfill import fill_named, name_seed, unit_fill
from tests import burgers_cases as KB
from tests.judging import SectionLog, rel_err
from tests.step_tail_cases import FLOOR_GATE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
LOG = SectionLog(os.path.join(ROOT, "profiles", "r21_darcy_errors.txt"))
FLOOR = FLOOR_GATE
CAP = 0.1
DATA_WEIGHT = 5.0
T = 16                                       # csrc/k_darcy_loss.h DARCY_T: residual cells per tile side
# (B, S): a single residual cell; two; three; one full tile; a second tile of one cell; a third tile of one cell; 37; the
# workload's grid; 141 (sub 3 of the 421-point data)
SHAPES = ((1, 5), (2, 6), (2, 7), (2, T + 4), (2, T + 5), (2, 2 * T + 5), (3, 37), (2, 61), (1, 141))
GOLDEN_CASES = (("white", (2, 7)), ("darcy", (2, 7)), ("white", (2, 37)), ("darcy", (2, 37)))
scalar_err = KB.scalar_err


def families(shape):
    return ("white", "darcy") if shape[1] >= 37 else ("white",)


def case_name(family, shape, mol=False, y=True):
    return f"darcy_loss {family} B={shape[0]} S={shape[1]}" + (" mol" if mol else "") + ("" if y else " no-y")


def mollifier(S):
    """train_2d.py:58 / eval_2d.py:27: float32 throughout, from the float32 mesh of torch2dgrid"""
    xs = torch.linspace(0, 1, steps=S)
    xx, yy = torch.meshgrid(xs, xs, indexing="ij")
    return torch.sin(np.pi * xx) * torch.sin(np.pi * yy) * 0.001


@functools.lru_cache(maxsize=None)
def make_inputs(family, shape):
    """{"out", "u", "a", "y" (B, S, S), "mol" (S, S)} float32 on the CPU"""
    B, S = shape
    tag = f"darcy.{family}.{B}.{S}"
    mol = mollifier(S)
    x = (np.arange(S, dtype=np.float64) / (S - 1))
    if family == "white":
        out = fill_named(tag + ".out", (B, S, S), 1.0, dtype=np.float64)
        a = 1.25 + 0.75 * fill_named(tag + ".a", (B, S, S), 1.0, dtype=np.float64)
        u = out
    elif family == "darcy":
        field, g = np.zeros((B, S, S)), np.zeros((B, S, S))
        for m in range(1, 4):
            for n in range(1, 4):
                cf = unit_fill((B,), name_seed(f"{tag}.a.{m}.{n}"))[:, None, None]
                ph = math.pi * unit_fill((B,), name_seed(f"{tag}.aphase.{m}.{n}"))[:, None, None]
                field += cf * np.cos(math.pi * m * x[None, :, None] + ph) * np.cos(math.pi * n * x[None, None, :] - ph)
                cg = unit_fill((B,), name_seed(f"{tag}.g.{m}.{n}"))[:, None, None]
                g += cg / (m * n) * np.sin(math.pi * m * x[None, :, None]) * np.sin(math.pi * n * x[None, None, :])
        a = np.where(field > 0, 12.0, 3.0)
        out = 8.0 + 3.0 * g
        u = (torch.from_numpy(out.astype(np.float32)) * mol).double().numpy()
    else:
        raise ValueError(family)
    y = u + 0.1 * math.sqrt(float((u * u).mean())) * fill_named(tag + ".y", (B, S, S), 1.0, dtype=np.float64)
    f32 = lambda v: torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32))      # noqa: E731
    return {"out": f32(out), "u": f32(u), "a": f32(a), "y": f32(y), "mol": mol}


# ---------------------------------------------------------------------------------------------------------------------
# the restatement, one dtype throughout, with the explicit adjoint
# ---------------------------------------------------------------------------------------------------------------------
FAULTS = ("h_slip", "a_centre", "a_transposed", "norm_rows", "adjoint_a_index", "adjoint_sign", "mol_backward", "tile_edge")


def _sh(t, dm, dn):
    """t[.., m + dm, n + dn], zero off the grid"""
    S = t.shape[-1]
    out = torch.zeros_like(t)
    ms, md = (slice(dm, S), slice(0, S - dm)) if dm >= 0 else (slice(0, S + dm), slice(-dm, S))
    ns, nd = (slice(dn, S), slice(0, S - dn)) if dn >= 0 else (slice(0, S + dn), slice(-dn, S))
    out[..., md, nd] = t[..., ms, ns]
    return out


def residual(pred, a, inv4h2, fault=None):
    """Du (B, S-4, S-4); differentiable (the restated training loop takes autograd through it)"""
    c = pred[:, 2:-2, 2:-2]
    if fault == "a_transposed":
        a = a.transpose(1, 2)
    if fault == "a_centre":
        axp = axm = ayp = aym = a[:, 2:-2, 2:-2]
    else:
        axp, axm, ayp, aym = a[:, 3:-1, 2:-2], a[:, 1:-3, 2:-2], a[:, 2:-2, 3:-1], a[:, 2:-2, 1:-3]
    fx = axp * (pred[:, 4:, 2:-2] - c) - axm * (c - pred[:, :-4, 2:-2])
    fy = ayp * (pred[:, 2:-2, 4:] - c) - aym * (c - pred[:, 2:-2, :-4])
    return -(fx + fy) * inv4h2


def restated(out, a, y, mol, dtype, g_data=DATA_WEIGHT, g_f=1.0, fault=None):
    """{"loss_f", "loss_data" (0-dim; loss_data only with y), "field" (B, S-4, S-4), "grad" (B, S, S) = d(g_data loss_data +
    g_f loss_f)/dout, "grad_f": the loss_f part alone}, everything in `dtype` on the CPU; y / mol may be None"""
    assert fault is None or fault in FAULTS
    out, a = out.to(dtype), a.to(dtype)
    B, S, _ = out.shape
    h = 1.0 / S if fault == "h_slip" else 1.0 / (S - 1)
    inv4h2 = 1.0 / (4.0 * h * h)
    rows = S - 2 if fault == "norm_rows" else S - 4
    pred = out if mol is None else out * mol.to(dtype)
    Du = residual(pred, a, inv4h2, fault)
    res = Du - 1.0
    nf = res.reshape(B, -1).norm(dim=1)
    res_ = {"loss_f": (nf / rows).mean(), "field": Du}
    r = torch.zeros_like(out)
    safe = torch.where(nf > 0, nf, torch.ones_like(nf))
    r[:, 2:-2, 2:-2] = g_f * res / (B * rows * safe)[:, None, None] * (nf > 0).to(dtype)[:, None, None]
    am_x, ap_x, am_y, ap_y = _sh(a, -1, 0), _sh(a, 1, 0), _sh(a, 0, -1), _sh(a, 0, 1)
    far = (ap_x, am_x, ap_y, am_y) if fault == "adjoint_a_index" else (am_x, ap_x, am_y, ap_y)
    up_x = far[1] * _sh(r, 2, 0)
    if fault == "tile_edge":                  # cells m = T, T + 1 take nothing from r[m + 2], which the next tile owns
        up_x = up_x.clone()
        up_x[:, T:T + 2] = 0.0
    gx = far[0] * _sh(r, -2, 0) + up_x - (ap_x + am_x) * r
    gy = far[2] * _sh(r, 0, -2) + far[3] * _sh(r, 0, 2) - (ap_y + am_y) * r
    dpred_f = (1.0 if fault == "adjoint_sign" else -1.0) * (gx + gy) * inv4h2
    dpred = dpred_f.clone()
    if y is not None:
        y = y.to(dtype)
        nd, ny = (pred - y).reshape(B, -1).norm(dim=1), y.reshape(B, -1).norm(dim=1)
        res_["loss_data"] = (nd / ny).mean()
        dpred = dpred + g_data * (pred - y) / (B * nd * ny)[:, None, None]
    chain = (lambda t: t) if mol is None or fault == "mol_backward" else (lambda t: t * mol.to(dtype))
    res_["grad"], res_["grad_f"] = chain(dpred), chain(dpred_f)
    return res_


def operands(inp, mol, y):
    """(out, a, y, mol) of a case in one of its four forms: with the mollifier `out` is the unmollified field"""
    return (inp["out"] if mol else inp["u"]), inp["a"], (inp["y"] if y else None), (inp["mol"] if mol else None)


@functools.lru_cache(maxsize=16)
def references(family, shape, mol=False, y=True, g_data=DATA_WEIGHT, g_f=1.0):
    """(inputs, ref64, ref32) of one case, computed once and shared; nobody writes into them"""
    inp = make_inputs(family, shape)
    ops = operands(inp, mol, y)
    return inp, restated(*ops, torch.float64, g_data, g_f), restated(*ops, torch.float32, g_data, g_f)


# ---------------------------------------------------------------------------------------------------------------------
# the judged quantities
# ---------------------------------------------------------------------------------------------------------------------
def _d(t):
    return t.detach().to(device="cpu", dtype=torch.float64)


def worst_row_err(a, ref64):
    """the largest relative L2 of one x row (over samples and y); a row whose truth is all zero counts absolutely"""
    a, b = _d(a), _d(ref64)
    den = (b * b).sum((0, 2)).sqrt()
    return float((((a - b) ** 2).sum((0, 2)).sqrt() / torch.where(den > 0, den, torch.ones_like(den))).max())


def ring(t):
    """the outer two-cell ring of (B, S, S), flattened: the cells the residual never covers"""
    mask = torch.ones(t.shape[-2:], dtype=torch.bool)
    mask[2:-2, 2:-2] = False
    return _d(t)[:, mask]


def own_loss_f(field, dtype):
    """mean_b ||field_b - 1|| / (S - 4) of a stored residual field, evaluated in `dtype`"""
    f = field.detach().cpu().to(dtype)
    return float(((f - 1.0).reshape(f.shape[0], -1).norm(dim=1) / f.shape[1]).mean())


def loss_rows(got, ref64, ref32):
    """judge_budget rows (name, err, err_ref32, floor) of got = {"loss_f", "field"[, "loss_data", "grad"]} against the
    float64 restatement, the float32 one as the yardstick.  loss_f is also held against the float64 mean of the engine's OWN
    stored field (the reduction alone; yardstick: the float32 evaluation of that field)."""
    own64 = own_loss_f(got["field"], torch.float64)
    rows = [("field", rel_err(got["field"], ref64["field"]), rel_err(ref32["field"], ref64["field"]), FLOOR),
            ("field worst row", worst_row_err(got["field"], ref64["field"]), worst_row_err(ref32["field"], ref64["field"]), FLOOR),
            ("loss_f vs own field", scalar_err(got["loss_f"], own64), scalar_err(own_loss_f(got["field"], torch.float32), own64), FLOOR),
            ("loss_f", scalar_err(got["loss_f"], ref64["loss_f"]), scalar_err(ref32["loss_f"], ref64["loss_f"]), FLOOR)]
    if "loss_data" in ref64:
        rows.append(("loss_data", scalar_err(got["loss_data"], ref64["loss_data"]), scalar_err(ref32["loss_data"], ref64["loss_data"]), FLOOR))
    if "grad" in got:
        rows += [("dout", rel_err(got["grad"], ref64["grad"]), rel_err(ref32["grad"], ref64["grad"]), FLOOR),
                 ("dout worst row", worst_row_err(got["grad"], ref64["grad"]), worst_row_err(ref32["grad"], ref64["grad"]), FLOOR),
                 ("dout outer ring", rel_err(ring(got["grad"]), ring(ref64["grad"])), rel_err(ring(ref32["grad"]), ring(ref64["grad"])), FLOOR)]
    capped = [name for name, _, ref, _ in rows if not ref < CAP]
    assert not capped, f"float32 yardstick at or above {CAP}: {capped}"
    return rows


def corner_blocks(t):
    """the four 2 x 2 corner blocks of (B, S, S), which the equation term never reaches"""
    return torch.stack([t[:, :2, :2], t[:, :2, -2:], t[:, -2:, :2], t[:, -2:, -2:]])


# ---------------------------------------------------------------------------------------------------------------------
# the model on an odd grid, and the loops: train_2d_operator (train_2d.py:13-116) and eval_2d.py restated on
# burgers_cases.fno2d_forward
# ---------------------------------------------------------------------------------------------------------------------
MODES = (4, 4, 3)
MODEL_X = (2, 37, 37, 3)
MODEL_PADS = {"pad0": [0., 0.], "pad_right": [0., 3 / 37]}
TRAIN_N, TRAIN_NX, TRAIN_SUB, TRAIN_PDE_SUB, TRAIN_BATCH = 8, 81, 4, 2, 4          # S = 21, pde_S = 41
TRAIN_CFG = {"train": {"xy_loss": 5.0, "f_loss": 1.0, "epochs": 3, "save_dir": "darcy_test", "save_name": "d.pt"}}
TRAIN_LR = 1e-3
BURGERS_VISC = 0.01


def model_params(tag):
    """name -> float32 / complex64 tensor for FNO2d(modes [4,4,3] both ways, layers [32]*4, fc_dim 128), filled by name"""
    from pde_policylearning_amd.libs.models.pino_models import FNO2d
    sd = FNO2d(modes1=list(MODES), modes2=list(MODES), fc_dim=128, layers=[32] * 4, in_dim=3, act="gelu").state_dict()
    p = {}
    for n, v in sd.items():
        scale = 1.0 / v.shape[0] if v.is_complex() else (0.1 if v.dim() == 1 else 1.0 / v.shape[1] ** 0.5)
        p[n] = torch.from_numpy(np.asarray(fill_named(f"darcy.{tag}.{n}", tuple(v.shape), scale, complex_=v.is_complex())))
    return p


def model_input():
    return torch.from_numpy(fill_named("input:darcy_fno2d.x", MODEL_X, 1.0))


@functools.lru_cache(maxsize=None)
def train_arrays():
    """{"coeff", "sol"} (8, 81, 81) float64: the darcy family's coefficient and mollified field on the raw grid"""
    inp = make_inputs("darcy", (TRAIN_N, TRAIN_NX))
    return {"coeff": inp["a"].double().numpy(), "sol": inp["u"].double().numpy()}


def _batches(ds, n):
    return [tuple(torch.stack(c) for c in zip(*[ds[i] for i in range(s, min(s + n, len(ds)))])) for s in range(0, len(ds), n)]


def restated_training(p, ds, form, dtype, cfg=TRAIN_CFG, lr=TRAIN_LR):
    """train_2d_operator on the restatements in `dtype`, batches of TRAIN_BATCH in dataset order, torch.optim.Adam.
    form "combo": (data_ic, u, pde_ic) items; "flow": (x, u).  Returns [(train_loss, f_loss, data_loss)]."""
    q = {k: v.requires_grad_(True) for k, v in KB.to_dtype(p, dtype).items()}
    opt = torch.optim.Adam(list(q.values()), lr=lr)
    w = cfg["train"]
    mol = mollifier(ds.mesh.shape[0]).to(dtype)
    pde_mol = mollifier(ds.pde_mesh.shape[0]).to(dtype) if form == "combo" else None
    model = lambda x: KB.fno2d_forward(q, x.to(dtype), MODES, MODES, [0., 0.])[..., 0]      # noqa: E731

    def f_term(pred, a):
        S = pred.shape[1]
        res = residual(pred, a.to(dtype), (S - 1) ** 2 / 4.0) - 1.0
        return (res.reshape(res.shape[0], -1).norm(dim=1) / (S - 4)).mean()

    def data_term(pred, u):
        B = u.shape[0]
        return ((pred - u).reshape(B, -1).norm(dim=1) / u.reshape(B, -1).norm(dim=1)).mean()
    hist = []
    for _ in range(w["epochs"]):
        tot = np.zeros(3)
        for batch in _batches(ds, TRAIN_BATCH):
            opt.zero_grad()
            if form == "combo":
                data_ic, u, pde_ic = batch
                data = data_term(model(data_ic) * mol, u.to(dtype))
                f = f_term(model(pde_ic) * pde_mol, pde_ic[..., 0])
            else:
                x, u = batch
                pred = model(x) * mol
                data, f = data_term(pred, u.to(dtype)), f_term(pred, x[..., 0])
            loss = w["xy_loss"] * data + w["f_loss"] * f
            loss.backward()
            opt.step()
            tot += np.array([float(loss.detach()), float(f.detach()), float(data.detach())]) * u.shape[0]
        hist.append(tuple(tot / len(ds)))
    return hist


def _stats(test_err, f_err):
    se = lambda v: float(np.std(v, ddof=1) / np.sqrt(len(v)))      # noqa: E731
    return float(np.mean(test_err)), se(test_err), float(np.mean(f_err)), se(f_err)


def restated_eval_darcy(p, ds, dtype):
    """eval_darcy's (mean_err, std_err, mean_f_err, std_f_err) in `dtype`, batches of TRAIN_BATCH"""
    q = KB.to_dtype(p, dtype)
    mol = mollifier(ds.mesh.shape[0])
    test_err, f_err = [], []
    for x, u in _batches(ds, TRAIN_BATCH):
        out = KB.fno2d_forward(q, x.to(dtype), MODES, MODES, [0., 0.])[..., 0]
        r = restated(out, x[..., 0], u, mol, dtype)
        test_err.append(float(r["loss_data"]))
        f_err.append(float(r["loss_f"]))
    return _stats(test_err, f_err)


def burgers_batches():
    """two batches (x (2, 12, 32, 3), y (2, 12, 32)) of the Burgers model test's kind"""
    return [KB.train_data(f"darcy_eval_burgers{i}") for i in (1, 2)]


def restated_eval_burgers(p, batches, dtype, visc=BURGERS_VISC):
    q = KB.to_dtype(p, dtype)
    test_err, f_err = [], []
    for x, y in batches:
        out = KB.fno2d_forward(q, x.to(dtype), KB.MODES1, KB.MODES2, [0., 0.]).reshape(y.shape)
        B = y.shape[0]
        yd = y.to(dtype)
        test_err.append(float(((out - yd).reshape(B, -1).norm(dim=1) / yd.reshape(B, -1).norm(dim=1)).mean()))
        f_err.append(float(KB.restated(out, x[:, 0, :, 0], visc, dtype)["loss_f"]))
    return _stats(test_err, f_err)
