"""What the channel MLP of an FNO block (use_mlp=True; k_channel_mlp.h, functional.channel_mlp, FNOBlocks / FNO) is held to
(a helper module, not a conftest): the float64 restatement of the op and of the model on top of oracle.fno_oracle, the case
tables, the error table and the judge.  Shared by tests/test_channel_mlp_host.py (CPU: the restatement against the reference's
stored float32 results), tests/test_channel_mlp_gpu.py and tests/test_channel_mlp_hygiene_gpu.py.

The reference (neuralop/models/fno_block.py:123-170, mlp.py:26-54, skip_connections.py:38-74; use_mlp=True, norm=None,
preactivation=False), per layer l of L with block input x:
    u  = gelu(spectral_conv_l(x) + fno_skip_l(x))        GELU on EVERY layer once there is an MLP (:147-150)
    t  = gelu(W1 u + b1)                                 mlp.fcs.0
    v  = gelu(W2 t + b2)                                 mlp.fcs.1 - activated too (mlp.py:49)
    y  = v + g * x                                       the MLP skip gates the block INPUT (:137, :162)
    x' = gelu(y) if l < L - 1 else y                     (:167-169)

Criterion (tests/judging.py, the float32-budget rule): err = relative L2 against the restatement in float64 on float64 copies
of the same float32 inputs; accepted when err == 0 or err < max(floor, 1.75 * err_ref32), err_ref32 being the same restatement
in float32 torch on the CPU.  Floors (those of tests/step_tail_cases.py): 2e-6 for fields and weight gradients, 2e-5 for the
reduced vectors db1, db2, dgate."""
import os
import re

import numpy as np
import torch
import torch.nn.functional as TF

from oracle import fno_oracle as O
from oracle.detfill import fill_named
from tests.judging import SectionLog, judge_budget, rel_err  # noqa: F401  (re-exported to the tests)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
LOG = SectionLog(os.path.join(ROOT, "profiles", "r18_channel_mlp_errors.txt"))
FLOOR_FIELD, FLOOR_VECTOR = 2e-6, 2e-5
WIDTHS = ((64, 32), (64, 64), (32, 32))          # (C, H) the kernels are built for
PARAMS = ("w1", "b1", "w2", "b2", "gate")


def floor_of(name):
    """op names (y, du, dx, dw1, ...) or state_dict names: sums over every pixel (bias and gate gradients) get the vector floor"""
    vector = name in ("db1", "db2", "dgate") or name.endswith(".bias") or re.fullmatch(r"fno_blocks\.mlp_skips\.\d+\.weight", name)
    return FLOOR_VECTOR if vector else FLOOR_FIELD


# ---------------------------------------------------------------------------------------------------------------------
# the op
# ---------------------------------------------------------------------------------------------------------------------
def mlp_op(u, x, w1, b1, w2, b2, gate=None, gelu_out=False):
    """y = [gelu](gelu(W2 gelu(W1 u + b1) + b2) + gate * x) in the dtype of its arguments (exact-erf GELU)"""
    t = TF.gelu(O.conv1x1(u, w1, b1))
    v = TF.gelu(O.conv1x1(t, w2, b2))
    y = v + (x if gate is None else gate.reshape(1, -1, *([1] * (x.dim() - 2))) * x)
    return TF.gelu(y) if gelu_out else y


# C, H, B, dims, what the case exercises
OP_CASES = [
    dict(name="one tile", C=64, H=32, B=1, dims=(8, 16)),
    dict(name="three tiles per sample", C=64, H=32, B=3, dims=(16, 24)),
    dict(name="3-D expansion 1", C=64, H=64, B=2, dims=(4, 8, 32)),
    dict(name="width 32", C=32, H=32, B=3, dims=(16, 24)),
    dict(name="896 tiles", C=64, H=32, B=7, dims=(128, 128)),
]


def op_inputs(case, scale=1.0, gate=True):
    """float32 CPU tensors: u, x uniform in +-scale, dy uniform in +-1, W1 / W2 uniform with unit gain (+-sqrt(3 / fan_in)),
    biases in +-0.5, the gate in +-1.7 (the fill the golden models give it)"""
    C, H, B, dims = case["C"], case["H"], case["B"], tuple(case["dims"])
    tag = f"cmlp.{C}.{H}.{B}.{'x'.join(map(str, dims))}."
    f = lambda n, shape, s: torch.from_numpy(fill_named(tag + n, shape, s))  # noqa: E731
    t = dict(u=f("u", (B, C) + dims, scale), x=f("x", (B, C) + dims, scale), dy=f("dy", (B, C) + dims, 1.0),
             w1=f("w1", (H, C), (3.0 / C) ** 0.5), b1=f("b1", (H,), 0.5), w2=f("w2", (C, H), (3.0 / H) ** 0.5), b2=f("b2", (C,), 0.5))
    if gate:
        t["gate"] = f("gate", (C,), 1.7)
    return t


def op_reference(t, gelu_out, dtype, x_grad=True):
    """the restatement and its gradients in `dtype` on the CPU: {y, du, dx, dw1, db1, dw2, db2[, dgate]}"""
    leaf = {k: v.detach().to(dtype).clone().requires_grad_(k != "x" or x_grad) for k, v in t.items() if k != "dy"}
    y = mlp_op(leaf["u"], leaf["x"], leaf["w1"], leaf["b1"], leaf["w2"], leaf["b2"], leaf.get("gate"), gelu_out)
    y.backward(t["dy"].to(dtype))
    out = {"y": y.detach(), "du": leaf["u"].grad}
    if x_grad:
        out["dx"] = leaf["x"].grad
    out.update({"d" + k: leaf[k].grad for k in PARAMS if k in leaf})
    return out


def op_engine(t, gelu_out, dev, x_grad=True):
    """functional.channel_mlp and its gradients on `dev`, same names as op_reference"""
    from pde_policylearning_amd import functional as F
    leaf = {k: v.detach().to(dev).requires_grad_(k != "x" or x_grad) for k, v in t.items() if k != "dy"}
    y = F.channel_mlp(leaf["u"], leaf["x"], leaf["w1"], leaf["b1"], leaf["w2"], leaf["b2"], leaf.get("gate"), gelu_out)
    y.backward(t["dy"].to(dev))
    out = {"y": y.detach(), "du": leaf["u"].grad}
    if x_grad:
        out["dx"] = leaf["x"].grad
    else:
        assert leaf["x"].grad is None
    out.update({"d" + k: leaf[k].grad for k in PARAMS if k in leaf})
    return out


def op_rows(got, ref32, ref64):
    return [(k, rel_err(got[k], r), rel_err(ref32[k], r), floor_of(k)) for k, r in ref64.items()]


# ---------------------------------------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------------------------------------
def fno_mlp_forward(p, x, n_modes, n_layers, fft_norm="forward"):
    """neuralop.models.FNO.forward with use_mlp=True on the pieces of oracle.fno_oracle; `p` maps the reference's state_dict
    names to tensors (a model without `mlp_skips.{l}.weight` has the identity skip)"""
    order = len(n_modes)
    half = [m // 2 for m in n_modes]
    nw = 2 ** (order - 1)
    h = O.conv1x1(x, p["lifting.fc.weight"], p["lifting.fc.bias"])
    for l in range(n_layers):
        ws = [O.complex_weight(p, f"fno_blocks.convs.weight.{nw * l + i}.tensor") for i in range(nw)]
        spec = O.spectral_conv_A(h, ws, p["fno_blocks.convs.bias"][l], half, fft_norm)
        u = TF.gelu(spec + O.conv1x1(h, p[f"fno_blocks.fno_skips.{l}.weight"]))
        m = f"fno_blocks.mlp.{l}.fcs."
        h = mlp_op(u, h, p[m + "0.weight"], p[m + "0.bias"], p[m + "1.weight"], p[m + "1.bias"],
                   p.get(f"fno_blocks.mlp_skips.{l}.weight"), gelu_out=l < n_layers - 1)
    h = TF.gelu(O.conv1x1(h, p["projection.fc1.weight"], p["projection.fc1.bias"]))
    return O.conv1x1(h, p["projection.fc2.weight"], p["projection.fc2.bias"])


# name: class, positional arguments, keyword arguments, input shape, golden file or None
MODEL_CASES = {
    "fno2d_mlp_small": ("FNO2d", (4, 4, 64), dict(n_layers=2, use_mlp=True), (2, 3, 16, 32), "fno2d_mlp_small.npz"),
    "fno3d_mlp_small": ("FNO3d", (4, 4, 4, 32), dict(n_layers=2, use_mlp=True, mlp_expansion=1.0), (1, 3, 4, 8, 32),
                        "fno3d_mlp_small.npz"),
    "fno2d_mlp_cfg2": ("FNO2d", (12, 12, 64), dict(n_layers=4, use_mlp=True), (2, 3, 32, 32), None),
}


def build_model(cname):
    """the package's model of a case (CPU, default initialisation)"""
    from pde_policylearning_amd.neuralop import models as M
    cls, pos, kw, _, _ = MODEL_CASES[cname]
    return getattr(M, cls)(*pos, **kw)


def model_params(cname, model=None):
    """-> ({state_dict name: float32 CPU tensor}, input, golden npz or None): parameters rebuilt as scale * unit_fill(name) with
    the golden file's scales (a case without one: 1.7 x the RMS of the model's own initialisation, as the generator does)"""
    _, _, _, shp, gfile = MODEL_CASES[cname]
    x = torch.from_numpy(fill_named("input:" + cname + ".x", shp, 1.0))
    if gfile is not None:
        g = np.load(os.path.join(GOLDEN, gfile))
        names = [k[len("scales/"):] for k in g.files if k.startswith("scales/")]
        p = {n: torch.from_numpy(fill_named(n, tuple(int(s) for s in g["shapes/" + n]), float(g["scales/" + n]))) for n in names}
        return p, x, g
    model = build_model(cname) if model is None else model
    p = {}
    for n, prm in model.named_parameters():
        rms = float(prm.detach().float().pow(2).mean().sqrt())
        p[n] = torch.from_numpy(fill_named(n, tuple(prm.shape), float(np.float32((rms if rms > 0 else 1.0) * 1.7))))
    return p, x, None


def model_reference(cname, p, x, dtype):
    """output and every parameter gradient of the restatement in `dtype` (loss y.square().sum())"""
    _, pos, kw, _, _ = MODEL_CASES[cname]
    leaf = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in p.items()}
    y = fno_mlp_forward(leaf, x.to(dtype), pos[:-1], kw["n_layers"])
    y.square().sum().backward()
    out = {"y": y.detach()}
    out.update({k: v.grad for k, v in leaf.items()})
    return out


def model_engine(cname, p, x, dev):
    """the package's model on `dev` with the parameters `p`: output and every parameter gradient, and the model"""
    model = build_model(cname)
    sd = model.state_dict()
    assert set(sd) == set(p), sorted(set(sd) ^ set(p))
    model.load_state_dict({k: v.reshape(sd[k].shape) for k, v in p.items()})
    model = model.to(dev)
    y = model(x.to(dev))
    y.square().sum().backward()
    out = {"y": y.detach()}
    out.update({k: v.grad for k, v in model.named_parameters()})
    return out, model
