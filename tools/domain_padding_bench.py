"""Time domain padding on the engine (functional.domain_pad / domain_crop: k_domain_pad, k_domain_crop) against
torch.nn.functional.pad and slicing, on the same GPU in the same process (GPU box).

  python tools/domain_padding_bench.py [--out profiles/r22_domain_padding_bench.txt] [--skip-model]

1. The ops alone, forward direction of each, at (64, 64, 128, 128) <-> 160 x 160 (one-sided 32) and (32, 32, 41, 41) <-> 45 x 45
   (one-sided 4): time, bytes moved / time (pad: the unpadded tensor read + the padded one written; crop: the interior read +
   the unpadded tensor written) and the fraction of the 6.3 TB/s a float4 copy achieves on this GPU (MI355X_MICROARCH.md).
   The torch versions are F.pad and slice + contiguous().
2. FNO2d(12, 12, 64) on 128 x 128, batch 64, domain_padding = 0.25, forward + backward, against the SAME model with the two
   kernels swapped for F.pad and slicing (a switch of this tool: the instance's pad / unpad are replaced; the product has no
   such switch).  The ratio is stated.

Method: the versions' results are compared bitwise (ops) / in relative L2 (model) at the timed shapes before anything is timed;
warm-up; then REPS blocks of ITERS calls per version, the versions taking turns inside every repetition; device events around
every block; median, min and max of the per-call times of the blocks."""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as TF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pde_policylearning_amd import _lib      # noqa: E402
from pde_policylearning_amd import functional as F      # noqa: E402

COPY_RATE = 6.3e12
REPS, WARM = 7, 3


def torch_pad(x, before, after):
    return TF.pad(x, [v for b, a in reversed(list(zip(before, after))) for v in (b, a)])


def torch_crop(y, before, after):
    return y[(Ellipsis,) + tuple(slice(b, y.shape[2 + d] - a) for d, (b, a) in enumerate(zip(before, after)))].contiguous()


def timed(fn, iters):
    """per-call ms over one block of `iters` calls"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def turns(versions, iters):
    """{name: per-call times of REPS blocks}, the versions alternating inside every repetition"""
    for fn in versions.values():
        timed(fn, WARM)
    out = {k: [] for k in versions}
    for _ in range(REPS):
        for k, fn in versions.items():
            out[k].append(timed(fn, iters))
    return out


def report(lines, label, times, nbytes=None):
    for k, v in times.items():
        med = statistics.median(v)
        rate = "" if nbytes is None else f"  {nbytes / med / 1e9:7.2f} TB/s = {100 * nbytes / (med * 1e-3) / COPY_RATE:3.0f} % of 6.3 TB/s"
        lines.append(f"  {label} {k:7s} median {med:8.4f} ms  min {min(v):8.4f}  max {max(v):8.4f}{rate}")
    e, t = statistics.median(times["engine"]), statistics.median(times["torch"])
    lines.append(f"  {label} torch / engine = {t / e:.2f} x")


def bench_ops(lines, dev, shape, p, iters):
    before, after = (0, 0), (p, p)
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.rand(*shape, generator=g, device=dev) * 2 - 1
    y = torch_pad(x, before, after)
    assert torch.equal(F.domain_pad(x, before, after).view(torch.int32), y.view(torch.int32))
    assert torch.equal(F.domain_crop(y, before, after).view(torch.int32), x.view(torch.int32))
    nbytes = 2 * x.numel() * 4
    lines.append(f"{tuple(shape)} <-> {tuple(y.shape[2:])}: {x.numel() * 4 / 1e6:.1f} MB unpadded, {y.numel() * 4 / 1e6:.1f} MB padded "
                 f"({REPS} blocks of {iters} calls)")
    report(lines, "pad ", turns({"engine": lambda: F.domain_pad(x, before, after), "torch": lambda: torch_pad(x, before, after)}, iters),
           (x.numel() + y.numel()) * 4)
    report(lines, "crop", turns({"engine": lambda: F.domain_crop(y, before, after), "torch": lambda: torch_crop(y, before, after)}, iters),
           nbytes)
    # the kernels alone (the engine's own event-bracketed launches): what is left of a call when the host's share is taken out
    L = _lib.lib()
    L.fno_profile_reset()
    L.fno_profile_enable(1)
    for _ in range(20):
        F.domain_pad(x, before, after)
        F.domain_crop(y, before, after)
    torch.cuda.synchronize()
    L.fno_profile_enable(0)
    for name, ms, n in _lib.profile_summary():
        moved = (x.numel() + y.numel()) * 4 if name == "k_domain_pad" else nbytes
        lines.append(f"  kernel {name:14s} {ms / n:8.4f} ms per launch over {n} launches (device events)  {moved / (ms / n) / 1e9:7.2f} TB/s")
    L.fno_profile_reset()


def bench_model(lines, dev, iters):
    from pde_policylearning_amd.neuralop.models import FNO2d
    torch.manual_seed(0)
    model = FNO2d(12, 12, 64, domain_padding=0.25).to(dev)
    x = torch.rand(64, 3, 128, 128, device=dev) * 2 - 1
    pad = model.domain_padding
    engine_pad, engine_unpad = pad.pad, pad.unpad

    def use(torch_ops):
        if torch_ops:
            before, after = pad.amounts((128, 128))
            pad.pad = lambda t: torch_pad(t, before, after)
            pad.unpad = lambda t: torch_crop(t, before, after)
        else:
            pad.pad, pad.unpad = engine_pad, engine_unpad

    def step(torch_ops):
        use(torch_ops)
        model.zero_grad(set_to_none=True)
        y = model(x)
        y.square().sum().backward()
        return y

    res = {}
    for name, flag in (("engine", False), ("torch", True)):
        y = step(flag)
        res[name] = [y.detach().clone()] + [q.grad.detach().clone() for q in model.parameters()]
    worst = max(float((a - b).norm() / b.norm()) for a, b in zip(res["engine"], res["torch"]))
    del res
    lines.append(f"FNO2d(12, 12, 64, domain_padding=0.25), batch 64, 128 x 128 -> 160 x 160, forward + backward ({REPS} blocks of {iters} steps)")
    lines.append(f"  engine pad / crop vs torch pad / slice: worst relative L2 over the output and every parameter gradient {worst:.3e}")
    report(lines, "step", turns({"engine": lambda: step(False), "torch": lambda: step(True)}, iters))
    use(False)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--skip-model", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    dev = torch.device("cuda:0")
    lines = [f"domain padding: functional.domain_pad / domain_crop against torch.nn.functional.pad / slicing, {torch.cuda.get_device_name(0)}"]
    bench_ops(lines, dev, (64, 64, 128, 128), 32, 50)
    bench_ops(lines, dev, (32, 32, 41, 41), 4, 200)
    if not a.skip_model:
        bench_model(lines, dev, 5)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
