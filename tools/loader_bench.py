"""Time the two ways a training loop gets its batches, on the same folder in the same process (GPU box):
  host    trainer.DevicePrefetcher over a torch DataLoader over libs.pde_data_loader (np.load + float64 encode per item,
          Python collate, pinned copy, .float() on the device) - what train_observer does without --device-data;
  device  libs.pde_data_loader.DeviceBatches (the folder's raw files resident on the GPU, one functional.data_gather launch per
          tensor).

  python tools/loader_bench.py [--out profiles/r25_device_data_bench.txt] [--n-planes 320] [--n-fields 64] [--skip-train]

Four workloads on synthetic float64 folders written to a temporary directory (page cache warm: one untimed epoch first):
planes 128 x 128 at batch 64, 32 x 32 crops of the same files at batch 20, sequences with T = 2 at batch 32, full fields
32 x 130 x 32 (U, W; V 32 x 129 x 32) with three target planes at batch 32.  Per workload: wall time of a whole epoch (the loop
only consumes the batches; one torch.cuda.synchronize() at the end) divided by its batches, EPOCHS_HOST / EPOCHS_DEV epochs of
each version taking turns, median, min and max; the one-off pool upload is reported on its own.  Every batch of the first
epoch is compared between the two versions before anything is timed.
Then the wall time of a train_observer epoch (train + test loop; FNO2dObserver(12, 12, 64), 128 x 128, batch 64, 256 train +
64 test samples) both ways from the loop's own `seconds`, first epoch dropped, and the engine's training step alone on a
resident batch of that shape - the figure a loader has to stay under for the step to bound the epoch."""
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
from pde_policylearning_amd import train_observer      # noqa: E402
from pde_policylearning_amd.libs.pde_data_loader import (DeviceBatches, FullFieldNSDataset, PDEDataset,      # noqa: E402
                                                         SequentialPDEDataset)
from pde_policylearning_amd.trainer import DevicePrefetcher      # noqa: E402

EPOCHS_HOST, EPOCHS_DEV = 3, 9


def write_planes(folder, n, size=128):
    rng = np.random.default_rng(0)
    meta = {}
    for tag in ("P_planes", "V_planes"):
        meta[tag] = dict(mean=0.3 + rng.standard_normal((size, size)), std=0.5 + rng.random((size, size)))
        for i in range(n):
            np.save(os.path.join(folder, f"{tag}_{i:06d}.npy"), rng.standard_normal((size, size)))
    np.save(os.path.join(folder, "metadata.npy"), meta, allow_pickle=True)


def write_fields(folder, n, grid=(32, 129, 32)):
    rng = np.random.default_rng(1)
    Nx, Ny, Nz = grid
    for tag, ny in (("U_field", Ny + 1), ("V_field", Ny), ("W_field", Ny + 1)):
        for i in range(n):
            np.save(os.path.join(folder, f"{tag}_{i:06d}.npy"), rng.standard_normal((Nx, ny, Nz)))
    meta = {"re": 178.1899, "U_field": {"dpdx": [0.0033] * n},
            "V_field": dict(mean=0.2 + rng.standard_normal((Nx, Ny, Nz)), std=0.5 + rng.random((Nx, Ny, Nz))),
            "P_planes": dict(mean=np.ones((Nx, Nz)), std=np.ones((Nx, Nz)))}
    np.save(os.path.join(folder, "metadata.npy"), meta, allow_pickle=True)


def epoch_ms(source):
    """(wall ms of one epoch, batches): the loop a trainer runs, minus the trainer"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n = 0
    for batch in source:
        n += 1
    del batch
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0), n


def same(a, b):
    return a.shape == b.shape and bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all())


def workload(name, ds, batch, dev, say):
    from torch.utils.data import DataLoader
    gen = lambda: torch.Generator().manual_seed(0)
    host = DevicePrefetcher(DataLoader(ds, batch_size=batch, shuffle=True, generator=gen()), dev)
    first = [tuple(t.clone() for t in b) for b in host]                 # (also warms the page cache)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    device = DeviceBatches(ds, batch, dev, True, gen())
    got = [tuple(t.clone() for t in b) for b in device]
    torch.cuda.synchronize()
    first_epoch = time.perf_counter() - t0
    assert len(got) == len(first) and all(same(x, y) for g, w in zip(got, first) for x, y in zip(g, w)), name
    del got, first
    times = {"host": [], "device": []}
    for rep in range(EPOCHS_DEV):
        if rep < EPOCHS_HOST:
            ms, n = epoch_ms(host)
            times["host"].append(ms / n)
        ms, n = epoch_ms(device)
        times["device"].append(ms / n)
    pool_mb = device.pool.planned_bytes() / 1e6
    med = {k: statistics.median(v) for k, v in times.items()}
    say(f"{name:44s} batch {batch:3d}, {n:3d} batches/epoch   host {med['host']:8.3f} ms/batch (min {min(times['host']):.3f}, max "
        f"{max(times['host']):.3f}; {batch / med['host']:.1f} k items/s)   device {med['device']:7.4f} ms/batch (min {min(times['device']):.4f}, "
        f"max {max(times['device']):.4f}; {batch / med['device']:.0f} k items/s)   ratio {med['host'] / med['device']:.0f} x   "
        f"pool {pool_mb:.0f} MB, first epoch with the upload {first_epoch:.2f} s")
    return med


def step_ms(dev, batch=64, size=128, iters=30):
    """the training step of train_observer's plane branch alone, on one resident batch"""
    from pde_policylearning_amd.libs.models.fno_models import FNO2dObserver
    from pde_policylearning_amd.trainer import FlatGradBucket, FusedAdam, FusedLpLoss, MeanStdDecoder, train_step
    model = FNO2dObserver(12, 12, 64).to(dev)
    bucket = FlatGradBucket(model.parameters(), direct_module=model, zero_all=False)
    opt = FusedAdam(bucket, lr=1e-3, weight_decay=1e-4)
    loss_fn = FusedLpLoss(size_average=False, decoder=MeanStdDecoder(np.zeros((size, size)), np.ones((size, size)), eps=1e-5, device=dev))
    p, v = torch.randn(batch, size, size, 1, device=dev), torch.randn(batch, size, size, device=dev)
    forward = lambda x: model(x, None)
    for _ in range(5):
        train_step(forward, bucket, opt, (p,), v, loss_fn)
    out = []
    for _ in range(5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            train_step(forward, bucket, opt, (p,), v, loss_fn)
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / iters)
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None)
    ap.add_argument("--n-planes", type=int, default=320)
    ap.add_argument("--n-fields", type=int, default=64)
    ap.add_argument("--skip-train", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say(f"device-resident training data against the host loader; {torch.cuda.get_device_name(0)}, torch {torch.__version__}, "
        f"{os.cpu_count()} host CPUs visible, torch threads {torch.get_num_threads()}")
    say(f"ms per batch = wall time of one epoch / batches; median (min, max) over {EPOCHS_HOST} host and {EPOCHS_DEV} device epochs taking turns")
    with tempfile.TemporaryDirectory() as tmp:
        planes, fields = os.path.join(tmp, "planes"), os.path.join(tmp, "fields")
        os.makedirs(planes)
        os.makedirs(fields)
        write_planes(planes, args.n_planes)
        write_fields(fields, args.n_fields)
        one, two = types.SimpleNamespace(model_timestep=1), types.SimpleNamespace(model_timestep=2)
        idx = list(range(args.n_planes))
        row1 = workload("planes 128 x 128 (float64 files)", PDEDataset(one, planes, idx, 1, 128, 128), 64, dev, say)
        workload("32 x 32 crops of the 128 x 128 files", PDEDataset(one, planes, idx, 1, 32, 32), 20, dev, say)
        workload("sequences T = 2 of 128 x 128 planes", SequentialPDEDataset(two, planes, idx, 1, 128, 128), 32, dev, say)
        workload("full fields 32 x 130 x 32, 3 target planes", FullFieldNSDataset(one, fields, list(range(args.n_fields)), [-10, -8, -6], 1, 32, 32),
                 32, dev, say)
        step = step_ms(dev)
        say(f"engine training step alone, FNO2dObserver(12, 12, 64), 128 x 128, batch 64, resident batch: {step:.3f} ms")
        verdict = "BELOW" if row1["device"] < step else "NOT below"
        say(f"first row: the device path's {row1['device']:.4f} ms per batch is {verdict} the engine's own step time of {step:.3f} ms "
            f"(the host loader's {row1['host']:.3f} ms is {row1['host'] / step:.1f} x the step)")
        if not args.skip_train:
            base = ["--data-folder", planes, "--ntrain", "256", "--ntest", "64", "--modes", "12", "--width", "64", "--x-range", "128",
                    "--y-range", "128", "--batch-size", "64", "--epochs", "4"]
            secs = {}
            for name, extra in (("host", []), ("device", ["--device-data"]), ("host again", []), ("device again", ["--device-data"])):
                hist = train_observer.run(train_observer.build_parser().parse_args(base + extra), log=lambda *_: None)
                secs[name] = [h["seconds"] for h in hist]
                say(f"train_observer epoch (4 train + 1 test batches of 64), {name:12s}: " + ", ".join(f"{s * 1e3:.1f}" for s in secs[name])
                    + f" ms per epoch; train rel-L2 of the last epoch {hist[-1]['train_l2']:.6f}")
            h, d = (statistics.median(secs[k][1:] + secs[k + " again"][1:]) for k in ("host", "device"))
            say(f"train_observer epoch, median without the first epochs: host {h * 1e3:.1f} ms, device {d * 1e3:.1f} ms, ratio {h / d:.1f} x "
                f"(5 batches: {h * 200:.2f} and {d * 200:.2f} ms per batch)")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
