"""Record tests/golden/domain_padding_ref.npz from the reference's own DomainPadding (neuralop/models/padding.py), loaded by
path from a checkout of the reference:

    python tools/make_domain_padding_golden.py --ref <reference checkout>

For every grid of tests/domain_padding_cases.py::GOLDEN_GRIDS (the grids on which the reference round-trips: every axis gets
the same amount) and both modes, the file holds `<key>/x`, `<key>/padded` = pad(x) and `<key>/unpadded` = unpad(pad(x)), and
nothing else.  The inputs are tests.domain_padding_cases.golden_input: small multiples of 1/4 with -0.0, NaN and both
infinities in front, so the file compresses to 16 KB and a comparison of bit images means something.  CPU only; no test
runs this."""
import argparse
import contextlib
import importlib.util
import io
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import domain_padding_cases as K  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="checkout of the reference (holds neuralop/models/padding.py)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "domain_padding_ref.npz"))
    args = ap.parse_args()
    spec = importlib.util.spec_from_file_location("reference_padding", os.path.join(args.ref, "neuralop", "models", "padding.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = {}
    for grid, frac in K.GOLDEN_GRIDS:
        for mode in K.MODES:
            x = K.golden_input(grid)
            pad = mod.DomainPadding(frac, mode)
            with contextlib.redirect_stdout(io.StringIO()):       # the reference prints every new resolution
                y = pad.pad(x)
            z = pad.unpad(y)
            assert z.shape == x.shape, (grid, frac, mode, tuple(y.shape), tuple(z.shape))
            key = K.golden_key(grid, frac, mode)
            out[key + "/x"], out[key + "/padded"], out[key + "/unpadded"] = x.numpy(), y.numpy(), z.numpy()
            print(f"{key}: {tuple(x.shape)} -> {tuple(y.shape)} -> {tuple(z.shape)}")
    np.savez_compressed(args.out, **out)
    print(f"wrote {args.out} ({os.path.getsize(args.out)} bytes)")


if __name__ == "__main__":
    main()
