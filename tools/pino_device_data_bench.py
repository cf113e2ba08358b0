"""Time the two ways train_pino gets its batches, on the same synthetic file in the same process (GPU box):
  host    trainer.DevicePrefetcher over a torch DataLoader over MultipleReynoldsKFaDataset (per item a torch.cat of the grid
          and the repeated initial plane, a strided collate of the permuted u, a pinned copy of the whole batch, host to
          device) - what train_pino does without --device-data;
  device  libs.pino_utils.datasets.DevicePinoBatches (the dataset's tensors resident on the GPU, one
          functional.data_transpose_gather and one functional.pino_input launch per batch).

  python tools/pino_device_data_bench.py [--out profiles/r26_pino_device_data_bench.txt] [--sizes 128 [256]] [--skip-train]
  python tools/pino_device_data_bench.py --kernels-only          # the three kernels alone, for a kernel-trace run around it

The file: a multi_reynolds_*.npz from a seed, raw S x S x 129, 8 trajectories; t_duration 0.5 gives 16 windows of S x S x 65;
batch 4 - the shipped fine-tuning shape at S = 128.
(1) per batch: wall clock around BATCHES batches of an endless sample_data stream ending in a device synchronise, BLOCKS
    blocks of each version taking turns after the first epoch of both was compared bit for bit; median, min, max.
(2) per training iteration: train_pino.train_ns with PINObserver2d([64] * 5, modes 8, fc_dim 128, pad_ratio 0.0625), loss
    5 IC + 1 PDE + 1 data, one model and optimizer, ITERS iterations per block, the option off and on taking turns after a
    warm-up block of each; the verdict compares on with off's own block-to-block spread.
(3) kernels: the two launches and, as the project's own yardstick, k_data_gather as a float32 cast-copy of the transpose's
    bytes, each bracketed by device events over REPS launches; bytes from shapes (transpose: read + write; input: write + a0;
    copy: read + write) and their share of 8 TB/s."""
import argparse
import os
import statistics
import sys
import tempfile
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pde_policylearning_amd import functional as F      # noqa: E402
from pde_policylearning_amd import train_pino      # noqa: E402
from pde_policylearning_amd.libs.pino_utils.datasets import DevicePinoBatches, MultipleReynoldsKFaDataset, sample_data      # noqa: E402
from pde_policylearning_amd.trainer import DevicePrefetcher, FlatGradBucket, FusedAdam, MultiStepLR      # noqa: E402

BATCHES, BLOCKS, ITERS, REPS, BATCH, TR, NTRAJ = 50, 7, 20, 20, 4, 129, 8
PEAK = 8e12


def write_file(folder, S):
    rng = np.random.default_rng(26)
    raw = rng.standard_normal((NTRAJ, TR, S, S), dtype=np.float32)
    path = os.path.join(folder, f"multi_reynolds_bench_{S}.npz")
    np.savez(path, data1=raw, data2=np.linspace(300, 500, NTRAJ).astype(np.float32))
    return path


def dataset(path, S):
    return MultipleReynoldsKFaDataset(paths=[path], raw_res=[S, S, TR], data_res=[S, S, TR], pde_res=[S, S, TR], n_samples=NTRAJ,
                                      offset=0, t_duration=0.5)


def sources(ds, dev, seed=0):
    from torch.utils.data import DataLoader
    gen = lambda: torch.Generator().manual_seed(seed)
    return (DevicePrefetcher(DataLoader(ds, batch_size=BATCH, shuffle=True, generator=gen()), dev),
            DevicePinoBatches(ds, BATCH, dev, True, gen()))


def block_ms(stream, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        batch = next(stream)
    del batch
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / n


def fmt(v, digits=3):
    return f"{statistics.median(v):.{digits}f} (min {min(v):.{digits}f}, max {max(v):.{digits}f})"


def per_batch(ds, S, dev, say):
    host, device = sources(ds, dev)
    first = [tuple(t.clone() for t in b) for b in host]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    got = [tuple(t.clone() for t in b) for b in device]
    torch.cuda.synchronize()
    upload = time.perf_counter() - t0
    assert len(got) == len(first) and all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for g, w in zip(got, first) for x, y in zip(g, w))
    del got, first
    hs, ds_ = sample_data(host), sample_data(device)
    times = {"host": [], "device": []}
    for _ in range(BLOCKS):
        times["host"].append(block_ms(hs, BATCHES))
        times["device"].append(block_ms(ds_, BATCHES))
    h, d = statistics.median(times["host"]), statistics.median(times["device"])
    say(f"per batch, {S} x {S} x 65, batch {BATCH} ({BATCH * S * S * 65 * 20 / 1e6:.0f} MB of u and a_in): host {fmt(times['host'])} ms   "
        f"device {fmt(times['device'], 4)} ms   ratio {h / d:.0f} x   first device epoch with the upload {upload * 1e3:.0f} ms")
    return h, d


def per_iteration(ds, S, dev, say):
    config = {"data": dict(pde_res=[S, S, TR], t_duration=0.5),
              "train": dict(start_iter=0, num_iter=ITERS, ic_loss=5.0, f_loss=1.0, xy_loss=1.0, save_step=10 ** 9, eval_step=10 ** 9),
              "log": dict(logdir="unused"),
              "model": dict(layers=[64] * 5, modes1=[8] * 4, modes2=[8] * 4, modes3=[8] * 4, fc_dim=128, act="gelu", pad_ratio=0.0625)}
    torch.manual_seed(0)
    model = train_pino.build_model(config, dev)
    bucket = FlatGradBucket(model.parameters(), direct_module=model)
    opt = FusedAdam(bucket, lr=1e-4)
    sched = MultiStepLR(opt, milestones=[10 ** 9], gamma=0.5)
    args = types.SimpleNamespace(log_every=10 ** 9)
    loaders = dict(zip(("off", "on"), (s if isinstance(s, DevicePinoBatches) else s.loader for s in sources(ds, dev))))

    def block(which):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        train_pino.train_ns(model, loaders[which], None, opt, sched, dev, config, args, log=lambda *_: None)
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / ITERS
    for which in ("off", "on"):
        block(which)                    # warm-up: plans, allocator, the upload
    times = {"off": [], "on": []}
    for _ in range(BLOCKS):
        for which in ("off", "on"):
            times[which].append(block(which))
    off, on = statistics.median(times["off"]), statistics.median(times["on"])
    spread = max(times["off"]) - min(times["off"])
    verdict = "NOT slower" if on <= off + spread else "SLOWER"
    say(f"per training iteration, {S} x {S} x 65, batch {BATCH}, blocks of {ITERS} iterations (each block pays one first batch): "
        f"off {fmt(times['off'])} ms   on {fmt(times['on'])} ms   off's own spread {spread:.3f} ms: on is {verdict} than off beyond it "
        f"(on - off = {on - off:+.3f} ms)")


def kernel_ms(call, label):
    """ms per launch of the kernel `label` inside `call`, from the library's event-bracketed launches"""
    from pde_policylearning_amd import _lib
    L = _lib.lib()
    torch.cuda.synchronize()
    L.fno_profile_reset()
    L.fno_profile_enable(1)
    try:
        for _ in range(REPS):
            call()
        torch.cuda.synchronize()
        return {name: ms / n for name, ms, n in _lib.profile_summary() if n}[label]
    finally:
        L.fno_profile_enable(0)
        L.fno_profile_reset()


def kernels(S, dev, say):
    T, n_src = 65, 2 * NTRAJ
    g = torch.Generator().manual_seed(1)
    frames = torch.randn(n_src, T, S * S, generator=g).to(dev)
    a0 = torch.randn(n_src, S, S, generator=g).to(dev)
    gx, gy, gt = (torch.linspace(0, 1, n).to(dev) for n in (S, S, T))
    idx = torch.tensor([11, 2, 7, 14])
    u, a_in, copy = (torch.empty(s, device=dev) for s in ((BATCH, S * S, T), (BATCH, S, S, T, 4), (BATCH, T, S * S)))
    moved = {"k_data_transpose_gather": 2 * 4 * u.numel(), "k_pino_input": 4 * a_in.numel() + 4 * BATCH * S * S,
             "k_data_gather<f32, cast> (copy)": 2 * 4 * copy.numel()}
    calls = {"k_data_transpose_gather": lambda: F.data_transpose_gather(frames, idx, out=u),
             "k_pino_input": lambda: F.pino_input(a0, idx, gx, gy, gt, out=a_in),
             "k_data_gather<f32, cast> (copy)": lambda: F.data_gather(frames, idx, (0, S * S, 1, T, S * S), out=copy)}
    for name, call in calls.items():
        for _ in range(3):
            call()
        ms = []
        for _ in range(5):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(REPS):
                call()
            b.record()
            torch.cuda.synchronize()
            ms.append(a.elapsed_time(b) / REPS)
        m = statistics.median(ms)
        k = kernel_ms(call, name.split("<")[0])
        say(f"kernel {name:34s} {S} x {S} x 65, {BATCH} entries: {moved[name] / 1e6:6.1f} MB moved; kernel alone {k * 1e3:7.1f} us "
            f"(the library's event-bracketed launch) = {moved[name] / (k * 1e-3) / 1e12:.2f} TB/s = {100 * moved[name] / (k * 1e-3) / PEAK:.0f} % "
            f"of 8 TB/s; {m * 1e3:7.1f} us per call with the index upload and the launch")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None)
    ap.add_argument("--sizes", type=int, nargs="+", default=[128])
    ap.add_argument("--skip-train", action="store_true")
    ap.add_argument("--kernels-only", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say(f"device-resident PINO training data against the host loader; {torch.cuda.get_device_name(0)}, torch {torch.__version__}, "
        f"torch threads {torch.get_num_threads()}; medians (min, max) over {BLOCKS} blocks taking turns")
    with tempfile.TemporaryDirectory() as tmp:
        for S in args.sizes:
            if not args.kernels_only:
                ds = dataset(write_file(tmp, S), S)
                per_batch(ds, S, dev, say)
                if not args.skip_train:
                    per_iteration(ds, S, dev, say)
                del ds
            kernels(S, dev, say)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
