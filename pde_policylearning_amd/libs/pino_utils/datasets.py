"""libs/pino_utils/datasets.py surface used by the PINO fine-tuning loop (train_pino.py:188-204):
`MultipleReynoldsKFaDataset` (:548-617) on the reference's files - an `.npz` with `data1` (N, T, S, S) vorticity
trajectories and `data2` (N,) Reynolds numbers when the path contains "multi_reynolds", otherwise one `.npy` whose
name carries `Re<digits>` - and `sample_data` (:24-27); and the Darcy sets of train_2d_operator / eval_darcy: `DarcyFlow`
(:368-387) and `DarcyCombo` (:416-442) on a MATLAB file with `coeff` and `sol` (N, nx, nx)."""
import re as _re

import numpy as np
import torch
from torch.utils.data import Dataset

from ..pde_data_loader import _RankIndexBatches
from .utils import get_grid3d, torch2dgrid


def sample_data(loader):
    """endless batches"""
    while True:
        yield from loader


class MultipleReynoldsKFaDataset(Dataset):
    """Items (u [S, S, T], a [S, S, T, 4] = (x, y, t, u(t = 0) repeated), Re).  With `t_duration` = 1/K every trajectory
    is cut into K windows that share their end points; the initial condition of window j is the raw frame j * step.
    As in the reference, window (i, j) gets `re[i]` counted from the START of the file, not from `offset` (:607-610)."""

    def __init__(self, paths, data_res, pde_res, raw_res, n_samples=None, total_samples=None, idx=0, offset=0, t_duration=1.0):
        super().__init__()
        self.data_res, self.pde_res, self.raw_res = data_res, pde_res, raw_res
        self.t_duration, self.paths, self.offset, self.n_samples = t_duration, paths, offset, n_samples
        self.T = self.pde_res[2] if t_duration == 1.0 else int(self.pde_res[2] * t_duration) + 1
        self.re = None
        self.load()
        if total_samples is not None:
            self.data = self.data[idx:idx + total_samples]
            self.a_data = self.a_data[idx:idx + total_samples]

    def load(self):
        path = self.paths[0]
        if 'multi_reynolds' in path:
            f = np.load(path)
            raw, self.re = f['data1'], f['data2']
        else:
            raw = np.load(path, mmap_mode='r')
            self.re = torch.tensor([int(_re.search(r'Re(\d+)', path).group(1))] * raw.shape[0]).float()
        sub_x = self.raw_res[0] // self.data_res[0]
        sub_t = (self.raw_res[2] - 1) // (self.data_res[2] - 1)
        a_sub_x = self.raw_res[0] // self.pde_res[0]
        rows = slice(self.offset, self.offset + self.n_samples)
        data = raw[rows, ::sub_t, ::sub_x, ::sub_x]
        if self.t_duration != 0.:
            end_t = self.raw_res[2] - 1
            K = int(1 / self.t_duration)
            data, self.re = self.partition(data)
            a = raw[rows, 0:end_t:end_t // K, ::a_sub_x, ::a_sub_x].reshape(self.n_samples * K, 1, self.pde_res[0], self.pde_res[1])
        else:
            a = raw[rows, 0:1, ::a_sub_x, ::a_sub_x]
        self.data = torch.from_numpy(np.ascontiguousarray(data)).to(torch.float32).permute(0, 2, 3, 1)        # [N, S, S, T]
        self.a_data = torch.from_numpy(np.ascontiguousarray(a)).to(torch.float32).permute(0, 2, 3, 1)[:, :, :, :, None]
        gx, gy, gt = get_grid3d(self.pde_res[1], self.T)
        self.grid = torch.cat((gx[0], gy[0], gt[0]), dim=-1)                                                  # S x S x T x 3

    def partition(self, data):
        """(N, T, S, S) -> (K N, T // K + 1, S, S) overlapping windows and their Reynolds numbers."""
        N, T, S = data.shape[:3]
        K = int(1 / self.t_duration)
        step = T // K
        out = np.zeros((K * N, step + 1, S, S))
        res = np.ones((K * N,))
        for i in range(N):
            for j in range(K):
                out[i * K + j] = data[i, j * step:(j + 1) * step + 1]
                res[i * K + j] = self.re if type(self.re) == int else self.re[i]
        return out, res

    def __getitem__(self, idx):
        a = torch.cat((self.grid, self.a_data[idx].repeat(1, 1, self.T, 1)), dim=-1)
        return self.data[idx], a, self.re[idx]

    def __len__(self):
        return self.data.shape[0]


class DevicePinoBatches(_RankIndexBatches):
    """Batches of a MultipleReynoldsKFaDataset assembled on the GPU from the dataset's own tensors, uploaded once: iterating
    yields the `(u (B, S, S, T), a_in (B, S, S, T, 4), re (B,))` float32 device tensors that
    `DevicePrefetcher(DataLoader(dataset, batch_size * world, shuffle, drop_last, generator))` followed by `shard_batch` yields,
    bit for bit, without per-item host work: no `torch.cat` of a grid that is the same for every item, no strided collate of
    the permuted `u`, no pinned copy of the whole batch.

    Pool: `dataset.data` in the (N, T, S, S) storage it is a permuted view of, `dataset.a_data` as (N, S, S) and `dataset.re`.
    Subsampling, windowing by `t_duration`, `offset`, `total_samples` and the Reynolds bookkeeping stay the host class's, done
    once at load.  u is one functional.data_transpose_gather launch, a_in one functional.pino_input launch from the three axis
    vectors of `dataset.grid` (checked here to reproduce the grid exactly), re a gather on the host of `batch` floats.
    Order: the index batches come from a DataLoader with the same arguments over an index-only dataset of the same length, so
    order, generator consumption, ragged tail and drop_last are the host loader's by construction.  Data parallelism: a rank
    gathers only its slice of the global batch.  A pool beyond `max_bytes` raises and the host loader remains the path."""

    def __init__(self, dataset, batch_size, device, shuffle, generator=None, drop_last=False, rank=0, world=1, max_bytes=8 << 30):
        if not isinstance(dataset, MultipleReynoldsKFaDataset):
            raise NotImplementedError(f"DevicePinoBatches: {type(dataset).__name__} (MultipleReynoldsKFaDataset)")
        self.dataset, self.device = dataset, torch.device(device)
        data, a = dataset.data, dataset.a_data
        grid = dataset.grid
        N = data.shape[0]
        self._index_loader(N, batch_size, shuffle, generator, drop_last, rank, world)
        if data.dim() != 4 or data.dtype != torch.float32 or a.dtype != torch.float32 or a.dim() != 5 or grid.dim() != 4 \
                or tuple(a.shape) != (N,) + tuple(grid.shape[:2]) + (1, 1) or grid.shape[3] != 3 or grid.dtype != torch.float32 \
                or len(dataset.re) < N:
            raise ValueError(f"DevicePinoBatches: data {tuple(data.shape)} {data.dtype}, a_data {tuple(a.shape)} {a.dtype}, grid "
                             f"{tuple(grid.shape)} {grid.dtype}, {len(dataset.re)} Reynolds numbers (float32 (N, S, S, T), "
                             "(N, S', S', 1, 1), (S', S', T', 3) and at least N expected)")
        need = 4 * (data.numel() + a.numel() + N)
        if need > max_bytes:
            raise MemoryError(f"device-resident data of {dataset.paths[0]}: the pool would hold {need} bytes, the budget is "
                              f"{int(max_bytes)} bytes (max_bytes; the host loader remains the path for such a dataset)")
        S1, S2, T = grid.shape[:3]
        self._axes = (grid[:, 0, 0, 0].clone(), grid[0, :, 0, 1].clone(), grid[0, 0, :, 2].clone())
        gx, gy, gt = self._axes
        again = torch.stack((gx[:, None, None].expand(S1, S2, T), gy[None, :, None].expand(S1, S2, T),
                             gt[None, None, :].expand(S1, S2, T)), dim=-1)
        if not torch.equal(again, grid):
            raise ValueError("DevicePinoBatches: dataset.grid is not the product of its three axis vectors (x along axis 0, y "
                             "along axis 1, t along axis 2); the host loader remains the path")
        self.shape = tuple(data.shape[1:])          # u: (S, S, T); a_in: the grid's (S', S', T', 4)
        self._re = torch.as_tensor(np.asarray(dataset.re)).float()      # the cast DevicePrefetcher makes on the device: one rounding
        self._pool = None

    def _resident(self):
        """(u pool (N, T, S * S), a0 pool (N, S, S), gx, gy, gt) on the device, uploaded at the first batch"""
        if self._pool is None:
            ds = self.dataset
            N, (S1, S2, T) = len(ds), self.shape
            frames = ds.data.permute(0, 3, 1, 2)      # the storage's own order: contiguous without a copy wherever load() made it
            self._pool = (frames.contiguous().view(N, T, S1 * S2).to(self.device),
                          ds.a_data.reshape((N,) + tuple(ds.grid.shape[:2])).to(self.device), *(g.to(self.device) for g in self._axes))
        return self._pool

    def __iter__(self):
        from ... import functional as F
        S1, S2, T = self.shape
        for items in self.index_batches():
            frames, a0, gx, gy, gt = self._resident()
            u = F.data_transpose_gather(frames, items).view(items.shape[0], S1, S2, T)
            yield u, F.pino_input(a0, items, gx, gy, gt), self._re[items].to(self.device)


def _darcy_arrays(datapath):
    """`coeff` and `sol` of a MATLAB file (scipy.io is needed for that alone), or of a mapping that holds both arrays"""
    if hasattr(datapath, 'keys'):
        return datapath['coeff'], datapath['sol']
    import scipy.io
    data = scipy.io.loadmat(datapath)
    return data['coeff'], data['sol']


def _darcy_points(nx, sub):
    return int(nx // sub) + 1 if sub > 1 else nx


class DarcyFlow(Dataset):
    """Items (x [S, S, 3] = (a, mesh x, mesh y), u [S, S]) of samples offset .. offset + num, every `sub`-th grid point:
    S = nx // sub + 1 (nx itself when sub is 1).  `mesh` is torch2dgrid(S, S)."""

    def __init__(self, datapath, nx, sub, offset=0, num=1):
        self.S = _darcy_points(nx, sub)
        a, u = _darcy_arrays(datapath)
        self.a = torch.tensor(np.asarray(a[offset: offset + num, ::sub, ::sub]), dtype=torch.float)
        self.u = torch.tensor(np.asarray(u[offset: offset + num, ::sub, ::sub]), dtype=torch.float)
        self.mesh = torch2dgrid(self.S, self.S)

    def __len__(self):
        return self.a.shape[0]

    def __getitem__(self, item):
        return torch.cat([self.a[item].unsqueeze(2), self.mesh], dim=2), self.u[item]


class DarcyCombo(Dataset):
    """Items (data_ic [S, S, 3], u [S, S], pde_ic [pde_S, pde_S, 3]): the coefficient with its solution on the data grid
    (every `sub`-th point) and the same coefficient alone on the equation grid (every `pde_sub`-th); `mesh`, `pde_mesh`.
    As in the reference, pde_S is nx when `sub` (not pde_sub) is 1 (:424)."""

    def __init__(self, datapath, nx, sub, pde_sub, num=1000, offset=0):
        super().__init__()
        self.S = _darcy_points(nx, sub)
        self.pde_S = int(nx // pde_sub) + 1 if sub > 1 else nx
        a, u = _darcy_arrays(datapath)
        self.a = torch.tensor(np.asarray(a[offset: offset + num, ::sub, ::sub]), dtype=torch.float)
        self.u = torch.tensor(np.asarray(u[offset: offset + num, ::sub, ::sub]), dtype=torch.float)
        self.mesh = torch2dgrid(self.S, self.S)
        self.pde_a = torch.tensor(np.asarray(a[offset: offset + num, ::pde_sub, ::pde_sub]), dtype=torch.float)
        self.pde_mesh = torch2dgrid(self.pde_S, self.pde_S)

    def __len__(self):
        return self.a.shape[0]

    def __getitem__(self, item):
        data_ic = torch.cat([self.a[item].unsqueeze(2), self.mesh], dim=2)
        pde_ic = torch.cat([self.pde_a[item].unsqueeze(2), self.pde_mesh], dim=2)
        return data_ic, self.u[item], pde_ic
