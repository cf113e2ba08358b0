"""Device-resident PINO training data, the part that needs no GPU: the argument checks of the two C entry points, the refusals
of functional.data_transpose_gather / pino_input, the order of DevicePinoBatches' index batches against a real DataLoader over
the dataset, the budget and grid refusals and the train_pino option."""
import ctypes
import types

import pytest
import torch

from tests import pino_device_data_cases as K


@pytest.fixture(scope="module")
def lib():
    from pde_policylearning_amd import build, _lib
    build.build()
    return _lib.lib()


P = ctypes.c_void_p(0x1000)       # never dereferenced
P4 = ctypes.c_void_p(0x1004)      # aligned to a float, not to an int64 or to 16 bytes
P1 = ctypes.c_void_p(0x1002)


def test_transpose_gather_refuses_bad_arguments_without_a_launch(lib):
    """every FNO_EINVAL / FNO_EUNSUPPORTED case of the header and count == 0; nothing is launched (this part runs without a
    GPU: a launch would be a HIP error, code FNO_EHIP, or a crash on the fake addresses)"""
    from pde_policylearning_amd import _lib
    EINVAL, EUNSUP = _lib.ABI.consts["FNO_EINVAL"], _lib.ABI.consts["FNO_EUNSUPPORTED"]
    assert "fno_data_transpose_gather" in _lib.EXPORTED_SYMBOLS
    names = ["src", "n_src", "rows", "cols", "idx", "count", "out", "out_stride", "stream"]
    ok = [P, 6, 5, 64, P, 4, P, 320, None]

    def call(**kw):
        assert set(kw) <= set(names)
        return lib.fno_data_transpose_gather(*[kw.get(n, a) for n, a in zip(names, ok)])
    with _lib.launch_log() as log:
        for name in ("src", "idx", "out"):
            assert call(**{name: None}) == EINVAL and b"null" in lib.fno_last_error(), name
        for kw in (dict(rows=0), dict(cols=0), dict(rows=-3), dict(cols=-1)):
            assert call(**kw) == EINVAL and b"at least 1 x 1" in lib.fno_last_error(), kw
        assert call(out_stride=319) == EINVAL and b"out_stride" in lib.fno_last_error()
        assert call(out_stride=0) == EINVAL
        for kw in (dict(src=P1), dict(out=P1), dict(idx=P4)):
            assert call(**kw) == EINVAL and b"aligned" in lib.fno_last_error(), kw
        assert call(n_src=2 ** 62, rows=1, cols=1, out_stride=1) == EUNSUP and b"2^62" in lib.fno_last_error()
        assert call(n_src=2 ** 52 + 1) == EUNSUP                           # (2^52 + 1) * 320 * 4 bytes
        assert call(count=2 ** 40, out_stride=2 ** 21) == EUNSUP and b"2^60" in lib.fno_last_error()
        # legal and empty: returns before a launch; a float's alignment is enough for src and out
        assert call(count=0) == 0
        assert call(count=0, src=P4, out=P4, out_stride=2 ** 40) == 0
        assert call(count=0, rows=1, cols=1, out_stride=1) == 0
    assert log.records == []


def test_pino_input_refuses_bad_arguments_without_a_launch(lib):
    from pde_policylearning_amd import _lib
    EINVAL, EUNSUP = _lib.ABI.consts["FNO_EINVAL"], _lib.ABI.consts["FNO_EUNSUPPORTED"]
    assert "fno_pino_input" in _lib.EXPORTED_SYMBOLS
    names = ["a0", "n_src", "idx", "count", "gx", "gy", "gt", "s1", "s2", "t", "out", "stream"]
    ok = [P, 6, P, 4, P, P, P, 8, 8, 5, P, None]

    def call(**kw):
        assert set(kw) <= set(names)
        return lib.fno_pino_input(*[kw.get(n, a) for n, a in zip(names, ok)])
    with _lib.launch_log() as log:
        for name in ("a0", "idx", "gx", "gy", "gt", "out"):
            assert call(**{name: None}) == EINVAL and b"null" in lib.fno_last_error(), name
        for kw in (dict(s1=0), dict(s2=0), dict(t=0), dict(s1=-1), dict(t=-7)):
            assert call(**kw) == EINVAL and b"at least 1 x 1 x 1" in lib.fno_last_error(), kw
        for kw in (dict(a0=P1), dict(gx=P1), dict(gy=P1), dict(gt=P1), dict(idx=P4)):
            assert call(**kw) == EINVAL and b"element size" in lib.fno_last_error(), kw
        for bad in (0x1004, 0x1008, 0x100c):
            assert call(out=ctypes.c_void_p(bad)) == EINVAL and b"16 bytes" in lib.fno_last_error(), bad
        assert call(n_src=2 ** 62, s1=1, s2=1) == EUNSUP and b"2^62" in lib.fno_last_error()
        assert call(count=2 ** 50) == EUNSUP and b"2^60" in lib.fno_last_error()          # 2^50 * 64 * 5 * 4 floats
        assert call(count=0) == 0
        assert call(count=0, a0=P4, gx=P4, gy=P4, gt=P4) == 0
        assert call(count=0, out=P4) == EINVAL                                            # (alignment is checked before the count)
    assert log.records == []


def test_functional_refuses_before_any_launch():
    """CPU tensors are refused naming the GPU; the index and `out` checks are the wrappers' own helpers, driven here with CPU
    tensors (only the anchor's device is read)"""
    from pde_policylearning_amd import functional as F
    pool = torch.zeros(5, 3, 16)
    idx = torch.tensor([0, 1])
    with pytest.raises(RuntimeError, match="GPU"):
        F.data_transpose_gather(pool, idx)
    with pytest.raises(RuntimeError, match="GPU"):
        F.pino_input(torch.zeros(5, 4, 4), idx, torch.zeros(4), torch.zeros(4), torch.zeros(3))
    with pytest.raises(RuntimeError, match="be a tensor"):
        F.data_transpose_gather([[1.0]], idx)
    for e in ("data_transpose_gather", "pino_input"):
        for bad in (-1, 5):
            with pytest.raises(RuntimeError, match=r"lie in \[0, 5\).*refused before anything is launched"):
                F._data_indices(e, torch.tensor([0, bad, 1]), 5)
        for bad in (torch.tensor([0, 1], dtype=torch.int32), torch.tensor([[0, 1]]), [0, 1], torch.tensor([0.0, 1.0])):
            with pytest.raises(RuntimeError, match="CPU int64 vector"):
                F._data_indices(e, bad, 5)
        assert F._data_indices(e, torch.tensor([0, 4, 4]), 5) == 3 and F._data_indices(e, torch.zeros(0, dtype=torch.int64), 5) == 0
    # out: size, dtype, device (the anchor's), density, alignment
    anchor = torch.zeros(1)
    buf = torch.zeros(2 * 16 * 3 + 8)
    assert F._data_out("x", None, anchor, (2, 16, 3)).shape == (2, 16, 3)
    got = F._data_out("x", buf[1:97], anchor, (2, 16, 3))
    assert got.shape == (2, 16, 3) and got.data_ptr() == buf.data_ptr() + 4
    with pytest.raises(RuntimeError, match="have 96 elements"):
        F._data_out("x", buf[:95], anchor, (2, 16, 3))
    with pytest.raises(RuntimeError, match="have 96 elements"):
        F._data_out("x", buf[:97], anchor, (2, 16, 3))
    with pytest.raises(RuntimeError, match="be torch.float32"):
        F._data_out("x", buf[:96].double(), anchor, (2, 16, 3))
    with pytest.raises(RuntimeError, match="be contiguous"):
        F._data_out("x", torch.zeros(96, 2)[:, 0], anchor, (2, 16, 3))
    with pytest.raises(RuntimeError, match="live on"):
        F._data_out("x", torch.zeros(96, device="meta"), anchor, (2, 16, 3))
    with pytest.raises(RuntimeError, match="be a tensor"):
        F._data_out("x", [0.0] * 96, anchor, (2, 16, 3))
    base = torch.zeros(96 + 8)
    lead = (-base.data_ptr() // 4) % 4                      # floats up to the first 16-byte boundary
    assert F._data_out("x", base[lead:lead + 96], anchor, (2, 4, 3, 4), align=16).shape == (2, 4, 3, 4)
    for off in (1, 2, 3):
        with pytest.raises(RuntimeError, match="16-byte boundary"):
            F._data_out("x", base[lead + off:lead + off + 96], anchor, (2, 4, 3, 4), align=16)


class _Recording(torch.utils.data.Dataset):
    """the dataset itself behind a record of which items a DataLoader asks for"""

    def __init__(self, ds):
        self.ds, self.seen = ds, []

    def __len__(self):
        return len(self.ds)

    def __getitem__(self, i):
        self.seen.append(int(i))
        return self.ds[i]


def _host_order(ds, batch, shuffle, drop_last, epochs=3):
    rec = _Recording(ds)
    loader = K.host_loader(rec, batch, shuffle, drop_last=drop_last)
    out = []
    for _ in range(epochs):
        for u, a, re in loader:
            items = rec.seen[-u.shape[0]:]
            assert torch.equal(u, ds.data[items]) and torch.equal(a[:, :, :, 0, 3], ds.a_data[items, :, :, 0, 0])
            out.append(items)
    return out


@pytest.fixture(scope="module")
def quarter(tmp_path_factory):
    return K.golden_dataset(tmp_path_factory.mktemp("kf"), "quarter_sub")


@pytest.mark.parametrize("shuffle", [False, True])
@pytest.mark.parametrize("drop_last", [False, True])
def test_index_batches_follow_the_dataloader(quarter, shuffle, drop_last):
    """12 items, batch 5, three epochs: the items of every batch, ragged tail or drop_last, are the ones a DataLoader with the same
    arguments asked the dataset for; building and ordering need no GPU"""
    from pde_policylearning_amd.libs.pino_utils.datasets import DevicePinoBatches
    assert len(quarter) == 12
    db = DevicePinoBatches(quarter, 5, "cuda:0", shuffle, K.generator() if shuffle else None, drop_last=drop_last)
    got = [b.tolist() for _ in range(3) for b in db.index_batches()]
    want = _host_order(quarter, 5, shuffle, drop_last)
    sizes = [5, 5] if drop_last else [5, 5, 2]
    assert got == want and [len(b) for b in got] == sizes * 3 and len(db) == len(sizes)
    assert all(b.dtype == torch.int64 and not b.is_cuda for b in db.index_batches())
    if shuffle:
        assert got[:len(sizes)] != got[len(sizes):2 * len(sizes)]          # (the generator moves on between epochs)
    if not drop_last:
        assert sorted(i for b in got[:3] for i in b) == list(range(12))


def test_index_batches_under_data_parallelism(quarter):
    """world = 2 with drop_last: the global batch of 6 is the host loader's and rank r gets shard_batch's slice of it"""
    from pde_policylearning_amd.libs.pino_utils.datasets import DevicePinoBatches
    from pde_policylearning_amd.trainer import shard_batch
    want = _host_order(quarter, 3 * 2, True, True)
    assert [len(b) for b in want] == [6] * 6
    for rank in (0, 1):
        db = DevicePinoBatches(quarter, 3, "cuda:0", True, K.generator(), drop_last=True, rank=rank, world=2)
        got = [b.tolist() for _ in range(3) for b in db.index_batches()]
        assert got == [shard_batch(torch.tensor(w), rank, 2).tolist() for w in want]
    with pytest.raises(ValueError, match="rank"):
        DevicePinoBatches(quarter, 3, "cuda:0", True, K.generator(), rank=2, world=2)


def test_pool_and_grid_refusals(tmp_path):
    from pde_policylearning_amd.libs.pde_data_loader import DeviceBatches
    from pde_policylearning_amd.libs.pino_utils.datasets import DevicePinoBatches
    ds = K.golden_dataset(tmp_path, "half")
    N, S, T = 4, 8, 5
    assert tuple(ds.data.shape) == (N, S, S, T) and ds.data.permute(0, 3, 1, 2).is_contiguous()      # the pool needs no host copy
    need = 4 * (N * S * S * T + N * S * S + N)
    with pytest.raises(MemoryError, match=rf"{need} bytes.*{need - 1} bytes"):
        DevicePinoBatches(ds, 3, "cuda:0", False, max_bytes=need - 1)
    db = DevicePinoBatches(ds, 3, "cuda:0", False, max_bytes=need)
    assert len(db) == 2 and db._pool is None                                                        # nothing uploaded yet
    gx, gy, gt = db._axes
    assert torch.equal(gx, ds.grid[:, 0, 0, 0]) and torch.equal(gy, ds.grid[0, :, 0, 1]) and torch.equal(gt, ds.grid[0, 0, :, 2])
    good = ds.grid
    for where in ((3, 2, 1, 0), (0, 5, 4, 1), (7, 7, 2, 2)):      # one entry of one channel off the product of the axis vectors
        ds.grid = good.clone()
        ds.grid[where] += 0.25
        with pytest.raises(ValueError, match="axis vectors"):
            DevicePinoBatches(ds, 3, "cuda:0", False)
    ds.grid = good[:, :, :, :2]
    with pytest.raises(ValueError, match="grid"):
        DevicePinoBatches(ds, 3, "cuda:0", False)
    ds.grid = good
    with pytest.raises(NotImplementedError, match="MultipleReynoldsKFaDataset"):
        DevicePinoBatches(torch.utils.data.TensorDataset(torch.zeros(3)), 3, "cuda:0", False)
    with pytest.raises(NotImplementedError, match="MultipleReynoldsKFaDataset"):      # DeviceBatches keeps its own dataset types
        DeviceBatches(ds, 3, "cuda:0", False, None)


def test_train_pino_option(tmp_path):
    import yaml
    from pde_policylearning_amd import train_pino as T
    off = T.build_parser().parse_args(["--config", "c.yaml"])
    assert off.device_data is False and off.device_data_max_gb == 8.0
    on = T.build_parser().parse_args(["--config", "c.yaml", "--device-data", "--device-data-max-gb", "0.5"])
    assert on.device_data is True and on.device_data_max_gb == 0.5
    plain = yaml.safe_load("data:\n  t_duration: 0.5\n")
    assert T.device_data_plan(plain, off) == (False, 8 << 30)
    assert T.device_data_plan(plain, on) == (True, 1 << 29)
    assert T.device_data_plan(plain, types.SimpleNamespace(seed=0)) == (False, 8 << 30)          # callers without the options
    wanted = yaml.safe_load("data:\n  t_duration: 0.5\n  device_data: true\n")
    assert T.device_data_plan(wanted, off) == (True, 8 << 30)
    # what the option selects, without a GPU: the loader kinds of run()
    ds = K.golden_dataset(tmp_path, "half")
    from torch.utils.data import DataLoader
    from pde_policylearning_amd.libs.pino_utils.datasets import DevicePinoBatches
    host = T._loader(ds, 3, "cuda:0", (False, 8 << 30), shuffle=True, drop_last=True, rank=1, world=2)
    assert isinstance(host, DataLoader) and host.batch_size == 6 and host.drop_last
    dev = T._loader(ds, 3, "cuda:0", (True, 8 << 30), shuffle=True, drop_last=True, rank=1, world=2)
    assert isinstance(dev, DevicePinoBatches) and (dev.rank, dev.world, dev.loader.batch_size, dev.loader.drop_last) == (1, 2, 6, True)
    with pytest.raises(MemoryError, match="budget"):
        T._loader(ds, 3, "cuda:0", (True, 100))
