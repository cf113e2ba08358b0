"""Generate tests/golden/fno2d_mlp_small.npz and fno3d_mlp_small.npz: the reference's FNO2d / FNO3d built with
use_mlp=True, run forward and backward on the CPU (float32), loss y.square().sum().

    python tools/make_channel_mlp_golden.py --ref DIR        # DIR: a checkout of the reference project

Runs where the reference is available; the stand-ins for its absent third-party imports and the deterministic fills are
oracle/make_golden.py's.  Each file holds DATA ONLY: the fill scale and the shape of every parameter, the output and every
parameter gradient.  Parameters and input are rebuilt from oracle.detfill on both sides (tests/channel_mlp_cases.py)."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle.make_golden import grads_of, input_fill, install_standins, refill_parameters, save  # noqa: E402

# name: (class name, positional arguments, keyword arguments, input shape)
CASES = {
    "fno2d_mlp_small": ("FNO2d", (4, 4, 64), dict(n_layers=2, use_mlp=True), (2, 3, 16, 32)),
    "fno3d_mlp_small": ("FNO3d", (4, 4, 4, 32), dict(n_layers=2, use_mlp=True, mlp_expansion=1.0), (1, 3, 4, 8, 32)),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    args = ap.parse_args()
    install_standins()
    sys.path.insert(0, args.ref)
    import neuralop.models as M
    torch.set_num_threads(8)
    for cname, (cls, pos, kw, shp) in CASES.items():
        torch.manual_seed(0)
        model = getattr(M, cls)(*pos, **kw)
        scales = refill_parameters(model)
        x = input_fill(cname + ".x", shp)
        y = model(x)
        y.square().sum().backward()
        save(os.path.join(args.out, f"{cname}.npz"), y=y, grads=grads_of(model), scales=scales,
             shapes={k: np.array(v.shape) for k, v in model.state_dict().items()})


if __name__ == "__main__":
    main()
