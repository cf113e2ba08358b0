"""Time forward + backward of a four-layer neuralop FNO1d on the engine (k_spec1d.h: three launches per spectral convolution and
direction, plus the pointwise kernel) against the same model composed from torch operations on the same GPU in the same
process, as the reference runs it: torch.fft.rfft, einsum, irfft, Conv1d, gelu (GPU box).

  python tools/fno1d_bench.py [--out profiles/r19_fno1d_bench.txt] [--shape burgers|long] [--blocks 7] [--iters 50]

Shapes: burgers  B 64, C 64, N 1024, n_modes 32 (16 kept bins)      long  B 16, C 32, N 8192, n_modes 64 (32 kept bins)
Method: both versions share one set of parameters; their outputs and parameter gradients are compared at the timed shape
first.  After warm-up the two versions take turns in BLOCKS blocks of ITERS steps (forward, then torch.autograd.grad of every
parameter), each block bracketed by device events; median, min and max of the per-step times.  Launches per engine step come
from the library's launch log (one extra step, outside the timed blocks).  For per-kernel times run this script once under
`rocprofv3 --kernel-trace --stats` (a run of its own: tracing slows the host)."""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as TF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pde_policylearning_amd import _lib      # noqa: E402
from pde_policylearning_amd.neuralop.models import FNO1d      # noqa: E402

SHAPES = {"burgers": dict(B=64, C=64, N=1024, n_modes=32), "long": dict(B=16, C=32, N=8192, n_modes=64)}
WARM = 5


def composed(model, x):
    """the model's forward from torch operations (tfno.py:195-211, fno_block.py:123-170, spectral_convolution.py:303-347)"""
    blk, convs, M = model.fno_blocks, model.fno_blocks.convs, model.fno_blocks.convs.half_n_modes[0]
    h = model.lifting(x)
    for l in range(model.n_layers):
        xf = torch.fft.rfft(h, norm=model.fft_norm)
        out = torch.zeros(h.shape[0], h.shape[1], h.shape[-1] // 2 + 1, dtype=xf.dtype, device=h.device)
        out[:, :, :M] = torch.einsum("bix,iox->box", xf[:, :, :M], torch.view_as_complex(convs.weight[l].tensor))
        h = torch.fft.irfft(out, n=h.shape[-1], norm=model.fft_norm) + convs.bias[l] + blk.fno_skips[l](h)
        if blk.gelu_after(l):
            h = TF.gelu(h)
    return model.projection(h)


def step(fn, model, x, dy, params):
    y = fn(model, x)
    return y, torch.autograd.grad(y, params, dy)


def block_ms(fn, model, x, dy, params, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        step(fn, model, x, dy, params)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def run(name, blocks, iters, dev):
    s = SHAPES[name]
    torch.manual_seed(0)
    model = FNO1d(s["n_modes"], s["C"], in_channels=2, out_channels=1).to(dev)
    params = list(model.parameters())
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.rand(s["B"], 2, s["N"], generator=g, device=dev) * 2 - 1
    dy = torch.rand(s["B"], 1, s["N"], generator=g, device=dev) * 2 - 1
    engine = lambda m, t: m(t)      # noqa: E731
    lines = [f"## {name}: B {s['B']}, C {s['C']}, N {s['N']}, n_modes {s['n_modes']} ({s['n_modes'] // 2} kept bins), 4 layers, "
             f"forward + backward, {torch.cuda.get_device_name(0)}"]
    ye, ge = step(engine, model, x, dy, params)
    yt, gt = step(composed, model, x, dy, params)
    rel = lambda p, q: float((p - q).norm() / q.norm())      # noqa: E731
    lines.append(f"  engine vs torch composition (float32 both): y rel L2 {rel(ye, yt):.3e}, worst parameter gradient "
                 f"{max(rel(p, q) for p, q in zip(ge, gt)):.3e}")
    del ye, ge, yt, gt
    with _lib.launch_log() as log:
        step(engine, model, x, dy, params)
        torch.cuda.synchronize()
    names = [r["variant"] or r["name"] for r in log.records]
    lines.append(f"  engine launches per step: {len(names)} ({sum(n.startswith('k_s1_') for n in names)} of the 1-D spectral kernels)")
    for fn in (engine, composed):
        block_ms(fn, model, x, dy, params, WARM)
    t = {"engine": [], "torch": []}
    for _ in range(blocks):
        for key, fn in (("engine", engine), ("torch", composed)):
            t[key].append(block_ms(fn, model, x, dy, params, iters))
    for key in ("engine", "torch"):
        v = t[key]
        lines.append(f"  {key:7s} median {statistics.median(v):.3f} ms per step  min {min(v):.3f}  max {max(v):.3f}  "
                     f"({blocks} blocks of {iters} steps)")
    ratio = statistics.median(t["torch"]) / statistics.median(t["engine"])
    lines.append(f"  torch composition / engine = {ratio:.2f} x")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--shape", default="", choices=[""] + list(SHAPES))
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--iters", type=int, default=50)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    dev = torch.device("cuda:0")
    lines = []
    for name in ([a.shape] if a.shape else list(SHAPES)):
        lines += run(name, a.blocks, a.iters, dev)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
