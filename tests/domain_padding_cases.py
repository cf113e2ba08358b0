"""What domain padding (k_domain_pad.h, functional.domain_pad / domain_crop, neuralop DomainPadding, FNO(domain_padding=f)) is
held to (a helper module, not a conftest): the restatement of the reference's pad / unpad and of the padded FNO.forward in the
dtype of its arguments, the case tables and the error table.  Shared by tests/test_domain_padding_host.py (CPU: the
restatement against the reference's recorded tensors, bit for bit), tests/test_domain_padding_gpu.py and
tests/test_domain_padding_hygiene_gpu.py.

The reference (neuralop/models/padding.py:35-95, tfno.py:195-211): p_d = int(round(f * r_d)) zeros per grid axis, behind the
interior ('one-sided') or on both sides ('symmetric'); FNO.forward = lifting, pad, the blocks on the extended grid, unpad,
projection.  Where every axis gets the same amount the restatement IS the reference (tests/golden/domain_padding_ref.npz);
where the amounts differ the reference's pad (torch's F.pad reads its list last dimension first) and unpad (slices in axis
order) disagree, and the restatement pads and crops axis d by its own p_d.

Criteria (tests/judging.py): the pad and crop ops are copies and are held BITWISE, as int32 images, against
torch.nn.functional.pad and slicing on the CPU.  Models: relative L2 against the restatement in float64 on float64 copies of the
same float32 inputs under the float32-budget rule, err == 0 or err < max(floor, 1.75 * err_ref32), with the floors of
tests/channel_mlp_cases.py (2e-6 fields and weight gradients, 2e-5 sums over every pixel)."""
import os

import numpy as np
import torch
import torch.nn.functional as TF

from oracle import fno_oracle as O
from oracle.detfill import fill_named
from tests.channel_mlp_cases import floor_of, mlp_op
from tests.judging import SectionLog, judge_budget, rel_err  # noqa: F401  (re-exported to the tests)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "domain_padding_ref.npz")
LOG = SectionLog(os.path.join(ROOT, "profiles", "r22_domain_padding_errors.txt"))
MODES = ("one-sided", "symmetric")

# grids on which the reference round-trips (every axis gets the same amount), recorded in both modes
GOLDEN_GRIDS = [((32, 32), 0.25), ((48, 48), 1.0 / 3.0), ((16, 16, 16), 1.0), ((41, 41), 0.1), ((9,), 0.34)]
GOLDEN_PADDED = {("one-sided", (32, 32)): (40, 40), ("one-sided", (48, 48)): (64, 64), ("one-sided", (16, 16, 16)): (32, 32, 32),
                 ("one-sided", (41, 41)): (45, 45), ("one-sided", (9,)): (12,), ("symmetric", (32, 32)): (48, 48),
                 ("symmetric", (48, 48)): (80, 80), ("symmetric", (16, 16, 16)): (48, 48, 48), ("symmetric", (41, 41)): (49, 49),
                 ("symmetric", (9,)): (15,)}
# grids on which it does not: grid, fraction, the padded grid of this package (one-sided)
NON_SQUARE = [((32, 64), 0.25, (40, 80)), ((8, 8, 12), 0.25, (10, 10, 15)), ((2, 40), 0.25, (2, 50))]


def golden_key(grid, frac, mode):
    return f"{'x'.join(map(str, grid))}_{frac:.4f}_{mode}"


def golden_input(grid):
    """(1, 1) + grid, float32: multiples of 1/4 in +-7.5 with -0.0, NaN, +Inf and -Inf in front.  The values repeat with
    period 61 - a prime that divides no extent and no padded extent of the recorded grids, so a tensor shifted by a row or a
    plane differs - which keeps the compressed file small (16 KB for its thirty arrays)"""
    n = int(np.prod(grid))
    v = ((np.arange(n, dtype=np.int64) * 37) % 61 - 30).astype(np.float32) / 4
    v[:4] = np.array([-0.0, np.nan, np.inf, -np.inf], dtype=np.float32)[:min(4, n)]
    return torch.from_numpy(v).reshape((1, 1) + tuple(grid))


def bits(t):
    """int32 image of a float32 tensor on the CPU: NaN equals NaN when the bits agree, -0.0 differs from +0.0"""
    return t.detach().to("cpu").contiguous().view(torch.int32)


# ---------------------------------------------------------------------------------------------------------------------
# the ops
# ---------------------------------------------------------------------------------------------------------------------
def amounts(grid, frac, mode):
    """(before, after) per axis for `grid`: p_d = int(round(f_d * r_d)) behind the interior, and in front of it too when
    symmetric; `frac` one fraction or one per axis"""
    fr = [float(frac)] * len(grid) if isinstance(frac, (float, int)) else [float(f) for f in frac]
    p = tuple(int(round(f * r)) for f, r in zip(fr, grid))
    assert mode in MODES
    return (p if mode == "symmetric" else (0,) * len(p)), p


def pad(x, before, after):
    """zeros around the grid of x (B, C, ...): torch's F.pad takes (before, after) pairs from the LAST axis backwards"""
    flat = [v for b, a in reversed(list(zip(before, after))) for v in (b, a)]
    return TF.pad(x, flat, mode="constant")


def unpad(y, before, after):
    return y[(Ellipsis,) + tuple(slice(b, y.shape[2 + d] - a) for d, (b, a) in enumerate(zip(before, after)))]


# name, tensor shape, before, after
OP_CASES = [
    ("1 one-sided", (2, 3, 9), (0,), (3,)),
    ("1 symmetric", (2, 3, 9), (3,), (3,)),
    ("2 nothing aligned", (2, 3, 5, 7), (0, 0), (2, 3)),
    ("2 symmetric", (2, 3, 5, 7), (2, 3), (2, 3)),
    ("3 env grid", (1, 1, 41, 41), (0, 0), (4, 4)),
    ("3 env grid symmetric", (1, 1, 41, 41), (4, 4), (4, 4)),
    ("4", (2, 32, 32, 32), (0, 0), (8, 8)),
    ("5 whole lines", (1, 64, 48, 48), (0, 0), (16, 16)),
    ("5 whole lines symmetric", (1, 64, 48, 48), (16, 16), (16, 16)),
    ("6 3-D", (2, 2, 4, 5, 6), (0, 0, 0), (1, 2, 3)),
    ("6 3-D symmetric", (2, 2, 4, 5, 6), (1, 2, 3), (1, 2, 3)),
    ("7 3-D", (1, 32, 16, 16, 16), (0, 0, 0), (16, 16, 16)),
    ("8 zero on the last axis", (2, 3, 6, 10), (0, 0), (3, 0)),
    ("8 zero on the first axis", (2, 3, 6, 10), (0, 2), (0, 2)),
    ("9 pads larger than the interior", (1, 2, 2, 3), (5, 5), (5, 5)),
    ("9 one-sided", (1, 2, 2, 3), (0, 0), (5, 5)),
    ("10 plain copy", (2, 3, 6, 10), (0, 0), (0, 0)),
    ("10 plain copy 1-D", (1, 1, 1), (0,), (0,)),
]
# the uneven work loop: more 16-byte quads than the largest launch has threads (8 workgroups of 256 per CU), not a multiple
UNEVEN_CASE = ("11 uneven loop", (4, 64, 90, 100), (0, 0), (7, 13))
GRID_PER_CU, BLOCK = 8, 256


def op_input(name, shape, specials=True):
    """float32 CPU tensor, uniform in +-1; with `specials` NaN, both infinities and -0.0 sit in the interior (first entries,
    last entry, and one in the middle)"""
    x = torch.from_numpy(fill_named("dompad.op." + name, shape, 1.0)).clone()
    if specials:
        v = x.view(-1)
        sp = torch.tensor([float("nan"), float("inf"), float("-inf"), -0.0])
        k = min(4, v.numel())
        v[:k] = sp[:k]
        if v.numel() > 8:
            v[-1] = -0.0
            v[v.numel() // 2] = float("nan")
    return x


def expected_launch(kernel, out_numel, ncu):
    """the launch-log record of one pad / crop call whose output (16-byte aligned) has `out_numel` elements"""
    nq = out_numel // 4
    grid = max(1, min((nq + BLOCK - 1) // BLOCK, GRID_PER_CU * ncu))
    return dict(name=kernel, variant=kernel, rb=0, ntiles=nq, grid=(grid, 1, 1), block=(BLOCK, 1, 1), lds=0)


# ---------------------------------------------------------------------------------------------------------------------
# the models
# ---------------------------------------------------------------------------------------------------------------------
def fno_padded_forward(p, x, n_modes, n_layers, frac, mode, use_mlp=False, fft_norm="forward"):
    """neuralop.models.FNO.forward with domain padding (tfno.py:195-211) on the pieces of oracle.fno_oracle, in the dtype of its
    arguments; `p` maps the reference's state_dict names to tensors.  Blocks without an MLP: fno_block.py:123-170 as
    oracle.fno_oracle.fno_forward states them; with one: the block of tests.channel_mlp_cases.fno_mlp_forward."""
    order = len(n_modes)
    half = [m // 2 for m in n_modes]
    nw = 2 ** (order - 1)
    h = O.conv1x1(x, p["lifting.fc.weight"], p["lifting.fc.bias"])
    before, after = amounts(tuple(h.shape[2:]), frac, mode)
    h = pad(h, before, after)
    for l in range(n_layers):
        ws = [O.complex_weight(p, f"fno_blocks.convs.weight.{nw * l + i}.tensor") for i in range(nw)]
        pre = O.spectral_conv_A(h, ws, p["fno_blocks.convs.bias"][l], half, fft_norm) + O.conv1x1(h, p[f"fno_blocks.fno_skips.{l}.weight"])
        if use_mlp:
            m = f"fno_blocks.mlp.{l}.fcs."
            h = mlp_op(TF.gelu(pre), h, p[m + "0.weight"], p[m + "0.bias"], p[m + "1.weight"], p[m + "1.bias"],
                       p.get(f"fno_blocks.mlp_skips.{l}.weight"), gelu_out=l < n_layers - 1)
        else:
            h = TF.gelu(pre) if O.fno_gelu_gate(l, n_layers) else pre
    h = unpad(h, before, after)
    h = TF.gelu(O.conv1x1(h, p["projection.fc1.weight"], p["projection.fc1.bias"]))
    return O.conv1x1(h, p["projection.fc2.weight"], p["projection.fc2.bias"])


# name: class, positional arguments, keyword arguments, input shape, padded grid.  B = 2 (3-D: 1), 4 layers, 3 in / 1 out
MODEL_CASES = {
    "tiled": ("FNO2d", (8, 8, 32), dict(domain_padding=1.0 / 3.0), (2, 3, 48, 48), (64, 64)),
    "tiled symmetric": ("FNO2d", (8, 8, 32), dict(domain_padding=0.5, domain_padding_mode="symmetric"), (2, 3, 32, 32), (64, 64)),
    "loose": ("FNO2d", (8, 8, 32), dict(domain_padding=0.25), (2, 3, 64, 64), (80, 80)),
    "unfused": ("FNO2d", (8, 8, 32), dict(domain_padding=0.25), (2, 3, 32, 32), (40, 40)),
    "non-square": ("FNO2d", (8, 8, 32), dict(domain_padding=0.25), (2, 3, 32, 64), (40, 80)),
    "mlp": ("FNO2d", (8, 8, 64), dict(domain_padding=1.0 / 3.0, use_mlp=True), (2, 3, 48, 48), (64, 64)),
    "3-D": ("FNO3d", (8, 8, 8, 32), dict(domain_padding=1.0), (1, 3, 16, 16, 16), (32, 32, 32)),
    "1-D": ("FNO1d", (16, 32), dict(domain_padding=0.5), (2, 3, 256), (384,)),
}
N_LAYERS = 4


def build_model(cname, **override):
    """the package's model of a case (CPU, default initialisation); `override` replaces keyword arguments"""
    from pde_policylearning_amd.neuralop import models as M
    cls, pos, kw, _, _ = MODEL_CASES[cname]
    return getattr(M, cls)(*pos, **{**kw, **override})


def model_params(cname):
    """-> ({state_dict name: float32 CPU tensor}, input): every parameter is scale * unit_fill(name) with scale = 1.7 x the RMS
    of the model's own initialisation (as tests.channel_mlp_cases does for a case without a golden file)"""
    shp = MODEL_CASES[cname][3]
    torch.manual_seed(0)
    p = {}
    for n, prm in build_model(cname).named_parameters():
        rms = float(prm.detach().float().pow(2).mean().sqrt())
        p[n] = torch.from_numpy(fill_named(n, tuple(prm.shape), float(np.float32((rms if rms > 0 else 1.0) * 1.7))))
    return p, torch.from_numpy(fill_named("input:dompad." + cname + ".x", shp, 1.0))


def model_reference(cname, p, x, dtype):
    """output, every parameter gradient and the input gradient ("dx") of the restatement in `dtype` (loss y.square().sum())"""
    _, pos, kw, _, _ = MODEL_CASES[cname]
    leaf = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in p.items()}
    xl = x.detach().to(dtype).clone().requires_grad_(True)
    y = fno_padded_forward(leaf, xl, pos[:-1], N_LAYERS, kw["domain_padding"], kw.get("domain_padding_mode", "one-sided"),
                           use_mlp=kw.get("use_mlp", False))
    y.square().sum().backward()
    out = {"y": y.detach(), "dx": xl.grad}
    out.update({k: v.grad for k, v in leaf.items()})
    return out


def load_model(cname, p, dev, **override):
    model = build_model(cname, **override)
    sd = model.state_dict()
    assert set(sd) == set(p), sorted(set(sd) ^ set(p))
    model.load_state_dict({k: v.reshape(sd[k].shape) for k, v in p.items()})
    return model.to(dev)


def model_engine(cname, p, x, dev):
    """the package's model on `dev` with the parameters `p`: output, every parameter gradient and dx, and the model"""
    model = load_model(cname, p, dev)
    xd = x.to(dev).requires_grad_(True)
    y = model(xd)
    y.square().sum().backward()
    out = {"y": y.detach(), "dx": xd.grad}
    out.update({k: v.grad for k, v in model.named_parameters()})
    return out, model


def model_rows(got, ref32, ref64):
    return [(k, rel_err(got[k], r), rel_err(ref32[k], r), floor_of(k)) for k, r in ref64.items()]
