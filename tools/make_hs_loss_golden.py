"""Generate tests/golden/hs_loss_small.npz from the reference, on the CPU in float32.

    python tools/make_hs_loss_golden.py --ref DIR        # DIR: a checkout of the reference project

The reference's own HsLoss (libs/utilities3.py:339-405, loaded by FILE PATH after oracle.make_golden.install_standins(): the
module imports libraries this project does not need) on the inputs tests/hs_loss_cases.py::golden_inputs rebuilds - shape
GOLDEN_SHAPE, fill names "hs.golden.x" / "hs.golden.y" with the scales stored under "scale/x", "scale/y" - and for every form
of hs_loss_cases.FORMS under mean, sum and reduction=False "<form>/<mean|sum|None>/value", the loss, and under mean
"<form>/mean/grad_even_rows", autograd's gradient on the grid rows 0, 2, 4 .. (half of it keeps the file under 100 KB; the
gradients under sum and reduction=False are the same array times the batch size).  k = 0 ungrouped is not a form: the
reference dies there inside torch.sqrt(int).

Runs where the reference is available.  The file holds DATA ONLY."""
import argparse
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle.make_golden import install_standins, save  # noqa: E402
from tests import hs_loss_cases as K  # noqa: E402


def load_utilities3(ref):
    install_standins()
    spec = importlib.util.spec_from_file_location("reference_utilities3", os.path.join(ref, "libs", "utilities3.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    args = ap.parse_args()
    u3 = load_utilities3(args.ref)
    torch.set_num_threads(8)
    x, y = K.golden_inputs()
    arrs = {"scale": {n: np.float64(v) for n, v in K.GOLDEN_SCALES.items()}, "shape": np.asarray(K.GOLDEN_SHAPE)}
    for k, a, group in K.FORMS:
        for red in K.REDUCTIONS:
            fn = u3.HsLoss(k=k, a=None if a is None else list(a), group=group, size_average=red == "mean", reduction=red is not None)
            leaf = x.clone().requires_grad_(True)
            value = fn(leaf, y)
            value.sum().backward()
            arrs[f"{K.form_id(k, a, group)}/{red}"] = {"value": value.detach().numpy()}
            if red == "mean":
                arrs[f"{K.form_id(k, a, group)}/{red}"]["grad_even_rows"] = leaf.grad[:, ::2].numpy()
    save(os.path.join(args.out, "hs_loss_small.npz"), **arrs)


if __name__ == "__main__":
    main()
