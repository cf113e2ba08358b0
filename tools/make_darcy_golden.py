"""Generate tests/golden/darcy_loss_small.npz from the reference, on the CPU in float32.

    python tools/make_darcy_golden.py --ref DIR        # DIR: a checkout of the reference project

The reference's own FDM_Darcy / darcy_loss (libs/pino_utils/losses.py:6-65, loaded by path: that module needs numpy and
torch alone) on the inputs of tests/darcy_cases.py::GOLDEN_CASES (`u` and `a` of each case, no mollifier, no data term):
the residual field, loss_f and autograd's gradient of loss_f, under "<family>_<B>_<S>/".

Runs where the reference is available.  The file holds DATA ONLY; inputs are rebuilt from oracle.detfill on both sides."""
import argparse
import importlib.util
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle.make_golden import save  # noqa: E402
from tests import darcy_cases as K  # noqa: E402


def load_losses(ref):
    spec = importlib.util.spec_from_file_location("reference_pino_losses", os.path.join(ref, "libs", "pino_utils", "losses.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    args = ap.parse_args()
    losses = load_losses(args.ref)
    torch.set_num_threads(8)
    arrs = {}
    for family, shape in K.GOLDEN_CASES:
        inp = K.make_inputs(family, shape)
        u = inp["u"].clone().requires_grad_(True)
        loss_f = losses.darcy_loss(u, inp["a"])
        loss_f.backward()
        arrs["{}_{}_{}".format(family, *shape)] = {"loss_f": loss_f.detach().numpy(), "du": u.grad.numpy(),
                                                   "field": losses.FDM_Darcy(inp["u"], inp["a"]).numpy()}
    save(os.path.join(args.out, "darcy_loss_small.npz"), **arrs)


if __name__ == "__main__":
    main()
