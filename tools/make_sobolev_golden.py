"""Generate tests/golden/sobolev_loss_small.npz from the reference, on the CPU in float32.

    python tools/make_sobolev_golden.py --ref DIR        # DIR: a checkout of the reference project

The reference's own LpLoss / H1Loss (neuralop/training/losses.py:62-277, loaded by FILE PATH: the package around it imports
libraries this project does not need, the module itself needs torch alone) on the white inputs of
tests/sobolev_cases.py::GOLDEN_SHAPES: the float32 inputs under "<shape>/x", "<shape>/y", and for every form
"<shape>/<H1|Lp>_<rel|abs>_<per|fix>_<sum|mean>/{value, grad}" the reduced loss and autograd's gradient of its sum.

Runs where the reference is available.  The file holds DATA ONLY."""
import argparse
import importlib.util
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle.make_golden import save  # noqa: E402
from tests import sobolev_cases as K  # noqa: E402


def load_losses(ref):
    spec = importlib.util.spec_from_file_location("reference_neuralop_losses", os.path.join(ref, "neuralop", "training", "losses.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def forms():
    """(key, loss name, relative, fixed, reduction)"""
    return [(f"{name}_{'rel' if rel else 'abs'}_{'fix' if fixed else 'per'}_{red}", name, rel, fixed, red)
            for name in ("H1", "Lp") for rel in (True, False) for fixed in ((False, True) if name == "H1" else (False,))
            for red in ("sum", "mean")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    args = ap.parse_args()
    losses = load_losses(args.ref)
    torch.set_num_threads(8)
    arrs = {}
    for shape, d in K.GOLDEN_SHAPES:
        x, y = K.make_inputs("white", shape, d)
        sid = K.shape_id(shape, d)
        arrs[sid] = {"x": x.numpy(), "y": y.numpy()}
        for key, name, rel, fixed, red in forms():
            if name == "H1":
                fn = losses.H1Loss(d=d, reductions=red, fix_x_bnd=fixed, fix_y_bnd=fixed, fix_z_bnd=fixed)
            else:
                fn = losses.LpLoss(d=d, p=2, reductions=red)
            leaf = x.clone().requires_grad_(True)
            value = fn.rel(leaf, y) if rel else fn.abs(leaf, y)
            value.sum().backward()
            arrs[sid][key + "/value"] = value.detach().numpy()
            arrs[sid][key + "/grad"] = leaf.grad.numpy()
    save(os.path.join(args.out, "sobolev_loss_small.npz"), **arrs)


if __name__ == "__main__":
    main()
