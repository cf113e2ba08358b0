"""Time the channel MLP of an FNO block (functional.channel_mlp: k_cmlp_fwd / k_cmlp_bwd) against the same computation composed
from torch operations, on the same GPU in the same process (GPU box).

  python tools/channel_mlp_bench.py [--batch 64] [--channels 64] [--hidden 32] [--size 128] [--out FILE]

Default shape: BASELINE config 2's block (B = 64, C = 64, H = 32, 128 x 128; 268 MB per tensor).
Versions:
  engine    functional.channel_mlp, forward, then torch.autograd.grad of (u, x, every parameter)
  torch     conv (kernel 1) -> F.gelu -> conv -> F.gelu -> + gate * x -> F.gelu, as the reference runs it, and its autograd
Method: warm-up, then REPS blocks of ITERS calls per version, the versions taking turns inside every repetition; forward and
backward are bracketed by device events; median, min and max of the per-call times of the blocks.  Before anything is timed
the two versions' results are compared at the timed shape.
Roofs (MI355X_MICROARCH.md: 8 TB/s HBM, 155 TFLOP/s fp32 matrix): forward 3 tensors and 4 C H flop per pixel, backward 5
tensors and 12 C H flop per pixel; the achieved fraction is the larger roof's time over the measured one."""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as TF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pde_policylearning_amd import functional as F      # noqa: E402

HBM, MATRIX = 8.0e12, 155.0e12
REPS, ITERS, WARM = 7, 10, 3
NAMES = ("u", "x", "w1", "b1", "w2", "b2", "gate")


def composed(u, x, w1, b1, w2, b2, gate, gelu_out):
    t = TF.gelu(TF.conv2d(u, w1[:, :, None, None], b1))
    v = TF.gelu(TF.conv2d(t, w2[:, :, None, None], b2))
    y = v + gate.reshape(1, -1, 1, 1) * x
    return TF.gelu(y) if gelu_out else y


def engine(u, x, w1, b1, w2, b2, gate, gelu_out):
    return F.channel_mlp(u, x, w1, b1, w2, b2, gate, gelu_out)


def timed(fn, t, dy, iters):
    """per-call (forward ms, backward ms) over `iters` calls"""
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3 * iters)]
    for i in range(iters):
        ev[3 * i].record()
        y = fn(*[t[k] for k in NAMES], True)
        ev[3 * i + 1].record()
        g = torch.autograd.grad(y, [t[k] for k in NAMES], dy)
        ev[3 * i + 2].record()
        del y, g
    torch.cuda.synchronize()
    f = sum(ev[3 * i].elapsed_time(ev[3 * i + 1]) for i in range(iters)) / iters
    b = sum(ev[3 * i + 1].elapsed_time(ev[3 * i + 2]) for i in range(iters)) / iters
    return f, b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--channels", type=int, default=64)
    ap.add_argument("--hidden", type=int, default=32)
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    dev = torch.device("cuda:0")
    B, C, H, S = a.batch, a.channels, a.hidden, a.size
    g = torch.Generator(device=dev).manual_seed(0)
    r = lambda *s: torch.rand(*s, generator=g, device=dev) * 2 - 1      # noqa: E731
    t = dict(u=r(B, C, S, S), x=r(B, C, S, S), w1=r(H, C) * (3 / C) ** 0.5, b1=r(H) * 0.5, w2=r(C, H) * (3 / H) ** 0.5, b2=r(C) * 0.5,
             gate=r(C) * 1.7)
    t = {k: v.requires_grad_(True) for k, v in t.items()}
    dy = r(B, C, S, S)
    lines = [f"channel MLP, B = {B}, C = {C}, H = {H}, {S} x {S} ({B * C * S * S * 4 / 1e6:.0f} MB per tensor), gelu_out = 1, "
             f"{torch.cuda.get_device_name(0)}"]
    # the two versions agree at the timed shape
    res = {}
    for name, fn in (("engine", engine), ("torch", composed)):
        y = fn(*[t[k] for k in NAMES], True)
        res[name] = [y.detach()] + [q.detach() for q in torch.autograd.grad(y, [t[k] for k in NAMES], dy)]
        del y
    for k, p, q in zip(("y",) + tuple("d" + n for n in NAMES), res["engine"], res["torch"]):
        lines.append(f"  engine vs torch composition (float32 both) {k:6s} rel L2 {float((p - q).norm() / q.norm()):.3e}")
    del res
    for fn in (engine, composed):
        timed(fn, t, dy, WARM)
    tf, tb = {"engine": [], "torch": []}, {"engine": [], "torch": []}
    for _ in range(REPS):
        for name, fn in (("engine", engine), ("torch", composed)):
            f, b = timed(fn, t, dy, ITERS)
            tf[name].append(f)
            tb[name].append(b)
    px = B * S * S
    roofs = {"forward": (3 * px * C * 4 / HBM * 1e3, 4 * C * H * px / MATRIX * 1e3),
             "backward": (5 * px * C * 4 / HBM * 1e3, 12 * C * H * px / MATRIX * 1e3)}
    for direction, times in (("forward", tf), ("backward", tb)):
        hbm, mat = roofs[direction]
        lines.append(f"{direction}: HBM roof {hbm:.3f} ms, fp32 matrix roof {mat:.3f} ms ({'HBM' if hbm >= mat else 'matrix'} is the larger)")
        for name in ("engine", "torch"):
            v = times[name]
            med = statistics.median(v)
            lines.append(f"  {name:7s} median {med:.3f} ms  min {min(v):.3f}  max {max(v):.3f}  ({REPS} blocks of {ITERS})"
                         + (f"  = {100 * max(hbm, mat) / med:.0f} % of the larger roof" if name == "engine" else ""))
        lines.append(f"  torch composition / engine = {statistics.median(times['torch']) / statistics.median(times['engine']):.2f} x")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
