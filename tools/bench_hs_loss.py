"""Time libs.utilities3.HsLoss on the engine, forward + backward, against the reference's own formula composed from torch
operations on the same GPU in the same process (GPU box).

  python tools/bench_hs_loss.py [--out profiles/r24_hs_loss_bench.txt] [--blocks 7] [--iters 200]

Shapes (64, 128, 128), (64, 64, 64), (32, 32, 32, 3) and (20, 64, 64, 8); the default form (k = 1, one weighted norm) and
k = 2 grouped, mean over the batch.  The composition is tests/hs_loss_cases.py::composed: two complex torch.fft.fftn calls,
the weights, torch.norm and autograd, as libs/utilities3.py:370-405 writes them.
Method, as tools/burgers_bench.py: outputs compared at the timed shape first; after warm-up the two versions take turns in
BLOCKS blocks of ITERS calls bracketed by device events; median, min and max, and the ratio of the medians.
Kernel times come from a second pass with the library's own event bracketing (fno_profile_enable: every launch between two
device events, a slow path that is never part of the timed blocks).  Achieved bytes/s is the ALGORITHMIC traffic - x and y
read once forward (8 bytes a cell), x and y read and dx written backward (12 bytes a cell) - over that kernel time; the
kernels are bound by their in-LDS transforms, so the figure states how far they are from a streaming kernel, not an HBM rate."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pde_policylearning_amd.libs.utilities3 import HsLoss      # noqa: E402
from tests import hs_loss_cases as K      # noqa: E402
from tools.bench_sobolev_loss import kernel_times      # noqa: E402
from tools.burgers_bench import alternate, rel      # noqa: E402

SHAPES = ((64, 128, 128), (64, 64, 64), (32, 32, 32, 3), (20, 64, 64, 8))
FORMS = (("default", 1, None, False), ("k=2 grouped", 2, (0.5, 0.25), True))


def bench(dev, shape, form, k, a, group, blocks, iters, lines):
    x, y = (t.to(dev) for t in K.make_inputs("white", shape))
    x.requires_grad_(True)
    loss = HsLoss(k=k, a=None if a is None else list(a), group=group)

    def engine():
        v = loss(x, y)
        return v, torch.autograd.grad(v, x)[0]

    def composed():
        v, _ = K.composed(x, y, k, a, group, "mean")
        return v, torch.autograd.grad(v, x)[0]
    (ve, ge), (vt, gt) = engine(), composed()
    name = f"{form} {tuple(shape)}"
    lines.append(f"  {name}: engine vs torch composition (float32 both): value rel {rel(ve.detach().reshape(-1), vt.detach().reshape(-1)):.3e}, "
                 f"dx rel L2 {rel(ge, gt):.3e}")
    alternate(name, engine, composed, blocks, iters, lines)
    cells = x.numel()
    t = kernel_times(engine, 20)
    for kern, nbytes in (("k_hs_plane_fwd", 8 * cells), ("k_hs_plane_bwd", 12 * cells)):
        lines.append(f"  {name}: {kern} {1e3 * t[kern]:.2f} us a launch (library event bracketing), algorithmic traffic {nbytes / 1e6:.2f} MB: "
                     f"{nbytes / (t[kern] * 1e-3) / 1e12:.3f} TB/s achieved")
    lines.append(f"  {name}: k_hs_finish {1e3 * t['k_hs_finish']:.2f} us a launch")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--iters", type=int, default=200)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    dev = torch.device("cuda:0")
    lines = [f"## libs.utilities3.HsLoss, forward + backward, mean over the batch, {torch.cuda.get_device_name(0)}"]
    for shape in SHAPES:
        for form, k, a, group in FORMS:
            bench(dev, shape, form, k, a, group, args.blocks, args.iters, lines)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
