"""Shapes, pools, dataset writers and the comparison for the device-resident PINO data tests (a helper module, not a test file).

The yardstick is the host path itself: `pool[idx].transpose(1, 2)` and the dataset's own `torch.cat((grid, a.repeat(...)), -1)`
for the two kernels, `DevicePrefetcher(DataLoader(MultipleReynoldsKFaDataset))` for whole batches.  Both kernels move words, so
every comparison is of int32 bit images and exact: NaN payloads and signs, infinities, both zeros and denormals included."""
import os

import numpy as np
import torch

# (rows, cols) of functional.data_transpose_gather: rows = frames of a window, cols = S * S
TRANSPOSE_SHAPES = [
    (1, 16),          # a copy
    (3, 16),          # below one tile
    (5, 64),          # odd rows; the golden file's shape
    (4, 4),
    (7, 225),         # cols no multiple of a tile or of 4: unaligned source rows, a last column block of 33
    (65, 1024),       # several column blocks, odd rows: the block's first float on every residue of a 16-byte line
    (129, 256),       # more frames than one LDS tile: the chunk loop, quads that run over a column's end
]
# (s1, s2, t) of functional.pino_input
INPUT_SHAPES = [(4, 4, 3), (8, 8, 5), (15, 15, 7), (32, 32, 65), (3, 5, 2)]
N_SRC = 6
IDX_VARIANTS = [[4], [5, 0, 3, 3, 1]]          # one entry; five with a repeated one

TG_COLS, PIN_POINTS = 64, 32                  # csrc/k_pino_batch.h: columns of a transpose tile, (x, y) points of an input workgroup


def transpose_launch(rows, cols, count):
    """the one launch of fno_data_transpose_gather as launch_log records it"""
    return {"name": "k_data_transpose_gather", "variant": "k_data_transpose_gather<chunked>" if rows > 128 else "k_data_transpose_gather<one tile>",
            "grid": (-(-cols // TG_COLS), count, 1), "block": (256, 1, 1)}


def input_launch(s1, s2, count):
    return {"name": "k_pino_input", "variant": "k_pino_input", "grid": (-(-(s1 * s2) // PIN_POINTS), count, 1), "block": (256, 1, 1)}


def assert_launched(log, want):
    """exactly the launches `want` (name, variant, grid, block), in order"""
    got = [{k: r[k] for k in ("name", "variant", "grid", "block")} for r in log.records]
    assert got == list(want), (got, want)


HOSTILE_WORDS = [0x7fc00000, 0x7fc00001, 0xffc12345, 0x7fffffff, 0xffffffff, 0x7f800000, 0xff800000, 0x00000000, 0x80000000,
                 0x00000001, 0x80000001, 0x007fffff, 0x00400000, 0x3fc00000, 0xc0100000]
# quiet NaNs with distinct payloads and both signs, +-inf, +-0, the smallest, the largest and a mid denormal, 1.5, -2.25


def pool(shape, seed, hostile=False):
    """a float32 CPU tensor of normal deviates; hostile: about a third of its words from HOSTILE_WORDS"""
    g = torch.Generator().manual_seed(seed)
    t = torch.randn(shape, generator=g)
    if hostile:
        words = torch.tensor(np.array(HOSTILE_WORDS, dtype=np.uint32).view(np.int32))
        pick = words[torch.randint(len(HOSTILE_WORDS), shape, generator=g)]
        iv = t.view(torch.int32)
        where = torch.rand(shape, generator=g) < 0.35
        iv[where] = pick[where]
    return t


def axes(s1, s2, t, seed=3, hostile=False):
    return tuple(pool((n,), seed + k, hostile) for k, n in enumerate((s1, s2, t)))


def host_input(a0, idx, gx, gy, gt):
    """the dataset's own expression per item (datasets.py __getitem__), stacked"""
    s1, s2, t = gx.numel(), gy.numel(), gt.numel()
    grid = torch.stack((gx[:, None, None].expand(s1, s2, t), gy[None, :, None].expand(s1, s2, t), gt[None, None, :].expand(s1, s2, t)), -1)
    return torch.stack([torch.cat((grid, a0[i].reshape(s1, s2, 1, 1).repeat(1, 1, t, 1)), dim=-1) for i in idx.tolist()])


def bits(t):
    return t.detach().contiguous().view(torch.int32).cpu()


def same_bits(a, b):
    """None when float32 tensors a and b hold the same words, else what differs"""
    if a.dtype != torch.float32 or b.dtype != torch.float32 or a.shape != b.shape:
        return f"{a.dtype} {tuple(a.shape)} against {b.dtype} {tuple(b.shape)}"
    d = bits(a) != bits(b)
    if bool(d.any()):
        w = torch.nonzero(d)[0].tolist()
        return (f"{int(d.sum())} of {a.numel()} words differ, first at {w}: {int(bits(a)[tuple(w)]) & 0xffffffff:#010x} against "
                f"{int(bits(b)[tuple(w)]) & 0xffffffff:#010x}")
    return None


def assert_batches_equal(got, want):
    """two lists of batches (tuples of tensors), one entry per batch of every epoch"""
    assert len(got) == len(want), (len(got), len(want))
    for n, (g, w) in enumerate(zip(got, want)):
        assert len(g) == len(w) == 3, (n, len(g), len(w))
        for k, (a, b) in enumerate(zip(g, w)):
            assert a.device == b.device, (n, k, a.device, b.device)
            msg = same_bits(a, b)
            assert msg is None, f"batch {n}, tensor {k}: {msg}"


# ----------------------------------------------------------------------------
# datasets
# ----------------------------------------------------------------------------
GOLDEN_CONFIGS = {"half": dict(data_res=[8, 8, 9], pde_res=[8, 8, 9], t_duration=0.5, n_samples=2, offset=1),
                  "quarter_sub": dict(data_res=[4, 4, 9], pde_res=[4, 4, 9], t_duration=0.25, n_samples=3, offset=0)}
GOLDEN_BATCH = {"half": 3, "quarter_sub": 5}          # 4 = 3 + 1 and 12 = 5 + 5 + 2 items: ragged tails


def golden_dataset(folder, tag):
    """the configurations of tests/golden/kf_dataset.npz, whose items test_kf_dataset_matches_reference_items holds to the
    reference's recorded ones"""
    from tests.util import load_golden
    from pde_policylearning_amd.libs.pino_utils.datasets import MultipleReynoldsKFaDataset
    g = load_golden("kf_dataset")
    path = os.path.join(folder, "multi_reynolds_tiny.npz")
    if not os.path.exists(path):
        np.savez(path, data1=g["raw"], data2=g["re_file"])
    return MultipleReynoldsKFaDataset(paths=[path], raw_res=[8, 8, 9], **GOLDEN_CONFIGS[tag])


SYNTH = dict(S=32, Tr=17, N=6)


def write_synthetic(folder):
    """the 32 x 32 x 17 multi-Reynolds file of tests/test_parity_gpu.py::test_train_pino_loop, from its seed"""
    rng = np.random.default_rng(2)
    S, Tr, N = SYNTH["S"], SYNTH["Tr"], SYNTH["N"]
    xs = np.linspace(0, 2 * np.pi, S, endpoint=False)
    X, Y = np.meshgrid(xs, xs, indexing="ij")
    raw = np.stack([[np.sin(X + 0.1 * t + p) * np.cos(2 * Y - 0.05 * t) + 0.3 * np.cos(4 * Y) for t in range(Tr)]
                    for p in rng.uniform(0, 6, N)]).astype(np.float32)
    path = os.path.join(folder, "multi_reynolds_synth.npz")
    np.savez(path, data1=raw, data2=np.linspace(300, 500, N).astype(np.float32))
    return path


def synthetic_config(path, logdir, num_iter=12):
    """The YAML keys of test_train_pino_loop; 12 iterations with evaluations at 0, 5 and 10, no checkpoint.  Width 32 and
    fc_dim 128 instead of that test's 16 and 32: the smallest model whose every layer runs on the engine's kernels, the ones
    documented as bitwise repeatable.  At width 16 the skip convolutions are torch's own Conv1d, whose weight gradient is not
    repeatable on the GPU: measured on one MI355X, four identical forward + backward calls on one batch gave identical losses
    and identical gradients for 32 of the 36 parameters, and `ws.0-3.weight` gradients that differed from call to call in 125
    to 239 of their 256 words - two host-loader runs then part ways at the first evaluation (val error 14.494991779 against
    14.494990826), which leaves nothing to hold the device path to."""
    S, Tr = SYNTH["S"], SYNTH["Tr"]
    return {
        "data": dict(train_paths=[path], test_paths=[path], offset=0, testoffset=4, n_data_samples=4, n_test_samples=2,
                     t_duration=0.5, raw_res=[S, S, Tr], data_res=[S, S, Tr], pde_res=[S, S, Tr]),
        "model": dict(layers=[32] * 5, modes1=[4] * 4, modes2=[4] * 4, modes3=[3] * 4, fc_dim=128, act="gelu", pad_ratio=0.0625),
        "train": dict(start_iter=0, batchsize=3, num_iter=num_iter, milestones=[6, 9], base_lr=0.004, scheduler_gamma=0.5,
                      ic_loss=5.0, f_loss=1.0, xy_loss=1.0, save_step=1000, eval_step=5),
        "test": dict(batchsize=2, data_res=[S, S, Tr]),
        "log": dict(logdir=str(logdir)),
    }


def synthetic_dataset(folder):
    from pde_policylearning_amd import train_pino
    path = write_synthetic(folder)
    S, Tr = SYNTH["S"], SYNTH["Tr"]
    return train_pino._dataset(synthetic_config(path, folder), [path], [S, S, Tr], 4, 0)          # 8 windows of 32 x 32 x 9


def generator(seed=7):
    return torch.Generator().manual_seed(seed)


def host_loader(ds, batch, shuffle, seed=7, drop_last=False):
    from torch.utils.data import DataLoader
    return DataLoader(ds, batch_size=batch, shuffle=shuffle, drop_last=drop_last, generator=generator(seed) if shuffle else None)
