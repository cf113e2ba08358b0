"""Time the Darcy PINO loss and step on the engine against the same computation composed from torch operations, on the same
GPU in the same process (GPU box).

  python tools/darcy_bench.py [--out profiles/r21_darcy_bench.txt] [--blocks 7] [--iters 50] [--only loss|step]

Shape: B 20, S 61 (421 points cut by 7), and S 211 (cut by 2: the equation grid of the three-tuple form) for the loss alone;
FNO2d(modes1=[20]*4, modes2=[20]*4, layers=[64]*5, fc_dim=128, in_dim=3), weights xy 5 / f 1.
  (a) loss   mollifier, data term and equation term, forward + backward: functional.darcy_loss (k_darcy_loss.h: two launches
             forward, one backward) against the torch sequence of the reference's loop (train_2d.py:75-82 with
             losses.py:6-65: the product with the mollifier, LpLoss, a ux and a uy by slices, their differences, LpLoss against
             ones, and their autograd twins).
  (b) step   the two-tuple step: model forward, the fused loss, backward, torch.optim.Adam, against the model composed from
             torch.fft.rfftn / einsum / irfftn / Conv1d / gelu (tools/burgers_bench.py torch_model) with the torch losses.  At
             S 61 the engine model runs its mixed route (spectral convolutions on the engine, pointwise parts torch modules),
             so the model part is expected to dominate and to differ little.
Method, as tools/burgers_bench.py: outputs compared at the timed shape first; after warm-up the two versions take turns in
BLOCKS blocks of ITERS steps bracketed by device events; median, min and max.  For per-kernel times run this script once under
`rocprofv3 --kernel-trace --stats` (a run of its own: tracing slows the host)."""
import argparse
import copy
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pde_policylearning_amd import functional as F      # noqa: E402
from pde_policylearning_amd.libs.models.pino_models import FNO2d      # noqa: E402
from pde_policylearning_amd.libs.pino_utils.train_2d import darcy_mollifier      # noqa: E402
from pde_policylearning_amd.libs.pino_utils.utils import torch2dgrid      # noqa: E402
from tools.burgers_bench import alternate, rel, torch_lploss, torch_model      # noqa: E402

B, S_DATA, S_PDE = 20, 61, 211
MODES, LAYERS = [20] * 4, [64] * 5
W_XY, W_F = 5.0, 1.0


def torch_darcy_loss(pred, a):
    """losses.py:6-65 from torch slices: a ux and a uy on the inner (S-2)^2 cells, differenced once more, LpLoss against ones"""
    n = pred.shape[1]
    two_h = 2.0 / (n - 1)
    inner = a[:, 1:-1, 1:-1]
    flux_x = inner * ((pred[:, 2:, 1:-1] - pred[:, :-2, 1:-1]) / two_h)
    flux_y = inner * ((pred[:, 1:-1, 2:] - pred[:, 1:-1, :-2]) / two_h)
    du = -((flux_x[:, 2:, 1:-1] - flux_x[:, :-2, 1:-1]) / two_h + (flux_y[:, 1:-1, 2:] - flux_y[:, 1:-1, :-2]) / two_h)
    return torch_lploss(du, torch.ones(du.shape, device=pred.device))


def inputs(dev, s):
    """x (B, s, s, 3) = (a, mesh), y (B, s, s): a two-valued coefficient (12 / 3) and a smooth field under the mollifier"""
    g = torch.Generator(device=dev).manual_seed(1)
    mesh = torch2dgrid(s, s).to(dev)
    ph = torch.rand(B, 2, 1, 1, generator=g, device=dev)
    field = torch.cos(3 * math.pi * (mesh[None, ..., 0] + ph[:, 0])) * torch.cos(2 * math.pi * (mesh[None, ..., 1] - ph[:, 1]))
    a = torch.where(field > 0, 12.0, 3.0)
    mol = darcy_mollifier(mesh)
    y = mol * (8.0 + 3.0 * torch.sin(math.pi * mesh[None, ..., 0] + ph[:, 0]) * torch.sin(2 * math.pi * mesh[None, ..., 1]))
    x = torch.cat((a.unsqueeze(-1), mesh.expand(B, s, s, 2)), -1)
    return x.contiguous(), y.contiguous(), mol.contiguous()


def bench_loss(dev, s, blocks, iters, lines):
    x, y, mol = inputs(dev, s)
    a = x[..., 0]
    out = (8.0 + 2.0 * torch.sin(5.0 * x[..., 1] + 3.0 * x[..., 2])).requires_grad_(True)

    def engine():
        ld, lf = F.darcy_loss(out, a, y, mol)
        return ld, lf, torch.autograd.grad(W_XY * ld + W_F * lf, out)[0]

    def composed():
        pred = out * mol
        ld, lf = torch_lploss(pred, y), torch_darcy_loss(pred, a)
        return ld, lf, torch.autograd.grad(W_XY * ld + W_F * lf, out)[0]
    (lde, lfe, ge), (ldt, lft, gt) = ([t.detach() for t in v] for v in (engine(), composed()))
    name = f"loss S {s}"
    lines.append(f"  {name}: engine vs torch composition (float32 both): loss_data {abs(float(lde) - float(ldt)) / float(ldt):.3e}, "
                 f"loss_f {abs(float(lfe) - float(lft)) / float(lft):.3e}, dout rel L2 {rel(ge, gt):.3e}")
    alternate(name, engine, composed, blocks, iters, lines)


def bench_step(dev, blocks, iters, lines):
    x, y, mol = inputs(dev, S_DATA)
    torch.manual_seed(0)
    me = FNO2d(modes1=MODES, modes2=MODES, layers=LAYERS, fc_dim=128, in_dim=3).to(dev)
    mt = copy.deepcopy(me)
    lines.append(f"  step: the engine covers lifting and layers at this shape: {me.route(x) == 'chain'}")
    with torch.no_grad():
        lines.append(f"  step: model output, engine vs torch composition on the same parameters: rel L2 {rel(me(x), torch_model(mt, x)):.3e}")
    oe, ot = torch.optim.Adam(me.parameters(), lr=1e-3), torch.optim.Adam(mt.parameters(), lr=1e-3)

    def engine():
        ld, lf = F.darcy_loss(me(x), x[..., 0], y, mol)
        total = W_XY * ld + W_F * lf
        oe.zero_grad()
        total.backward()
        oe.step()
        return total

    def composed():
        pred = torch_model(mt, x).squeeze(-1) * mol
        total = W_XY * torch_lploss(pred, y) + W_F * torch_darcy_loss(pred, x[..., 0])
        ot.zero_grad()
        total.backward()
        ot.step()
        return total
    te, tt = float(engine()), float(composed())
    lines.append(f"  step: total loss of the first step, engine {te:.6e} vs torch composition {tt:.6e}: {abs(te - tt) / abs(tt):.3e}")
    alternate("step", engine, composed, blocks, iters, lines)
    te, tt = float(engine()), float(composed())
    lines.append(f"  step: total loss after the timed steps, engine {te:.6e} vs torch composition {tt:.6e}: {abs(te - tt) / abs(tt):.3e}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--only", default="", choices=["", "loss", "step"])
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--iters", type=int, default=50)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    dev = torch.device("cuda:0")
    lines = [f"## Darcy PINO: B {B}, S {S_DATA} (loss also S {S_PDE}), FNO2d modes {MODES} layers {LAYERS} fc_dim 128, "
             f"weights xy {W_XY:g} / f {W_F:g}, {torch.cuda.get_device_name(0)}"]
    if args.only in ("", "loss"):
        bench_loss(dev, S_DATA, args.blocks, args.iters, lines)
        bench_loss(dev, S_PDE, args.blocks, args.iters, lines)
    if args.only in ("", "step"):
        bench_step(dev, args.blocks, args.iters, lines)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
