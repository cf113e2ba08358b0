"""Plane datasets with the reference surface and on-disk format (libs/pde_data_loader.py:8-127):
a folder of per-timestep `P_planes_######.npy` / `V_planes_######.npy` files (or `P_plane` / `V_plane`) and a pickled
`metadata.npy` dict holding per-field `mean` / `std` arrays (run_control.py:234-292 writes them).
Items are normalised on the host exactly as the reference does; trainer.DevicePrefetcher moves batches to the GPU
asynchronously (pinned staging + a copy stream) instead of the reference's per-step `.cuda().float()`
(run_pde_observers.py:173).  DeviceBatches is the device-resident alternative: the raw files of a folder are uploaded once and
every batch is assembled on the GPU by functional.data_gather, bit for bit what the host path delivers."""
import os
import weakref

import numpy as np
import torch
from torch.utils.data import DataLoader, Dataset

from .utilities3 import NormalizerGivenMeanStd


def _plane_names(metadata):
    if 'P_planes' in metadata:
        return 'P_planes', 'V_planes'
    if 'P_plane' in metadata:
        return 'P_plane', 'V_plane'
    raise RuntimeError("Not recognized key name!")


class _PlaneFolder(Dataset):
    def _open(self, data_folder, data_index, downsample_rate, x_range, y_range, use_patch):
        self.data_folder = data_folder
        self.downsample_rate, self.x_range, self.y_range = downsample_rate, x_range, y_range
        self.metadata = np.load(os.path.join(data_folder, 'metadata.npy'), allow_pickle=True).tolist()
        self.file_list = os.listdir(data_folder)
        p_name, v_name = _plane_names(self.metadata)
        self.p_plane_files = sorted(f for f in self.file_list if p_name in f)
        self.v_plane_files = sorted(f for f in self.file_list if v_name in f)
        self.p_plane_mean, self.p_plane_std = self.metadata[p_name]['mean'], self.metadata[p_name]['std']
        self.v_plane_mean, self.v_plane_std = self.metadata[v_name]['mean'], self.metadata[v_name]['std']
        self.data_index = data_index
        self.data_length = len(data_index)
        self.use_patch = use_patch
        crop = self._crop_stats
        self.p_norm = NormalizerGivenMeanStd(crop(self.p_plane_mean), crop(self.p_plane_std))
        self.v_norm = NormalizerGivenMeanStd(crop(self.v_plane_mean), crop(self.v_plane_std))

    def _crop_stats(self, a):
        if self.use_patch:                                           # pde_data_loader.py:31-35
            return a.reshape(-1, self.x_range, self.y_range).mean(0)
        d = self.downsample_rate                                      # :37-40
        return a[::d, ::d][:self.x_range, :self.y_range]

    def _load_plane(self, name, norm):
        t = torch.tensor(np.load(os.path.join(self.data_folder, name)))
        if self.use_patch:                                            # :54-57
            t = t.reshape(-1, self.x_range, self.y_range)
        else:
            d = self.downsample_rate
            t = t[::d, ::d][:self.x_range, :self.y_range]
        return norm.encode(t)


class PDEDataset(_PlaneFolder):
    """(p_plane, v_plane), each (X, Y, 1), normalised  (pde_data_loader.py:8-69)."""

    def __init__(self, args, data_folder, data_index, downsample_rate, x_range, y_range, use_patch=False, full_field=False):
        super().__init__()
        self._open(data_folder, data_index, downsample_rate, x_range, y_range, use_patch)

    def __len__(self):
        return self.data_length

    def __getitem__(self, index):
        i = self.data_index[index]
        return (self._load_plane(self.p_plane_files[i], self.p_norm).unsqueeze(-1),
                self._load_plane(self.v_plane_files[i], self.v_norm).unsqueeze(-1))


class SequentialPDEDataset(_PlaneFolder):
    """(p, v), each (timestep, X, Y): `args.model_timestep` consecutive planes  (pde_data_loader.py:72-127;
    the reference reads self.p_plane_* without ever setting them in this class - they are set here)."""

    def __init__(self, args, data_folder, data_index, downsample_rate, x_range, y_range, use_patch=False, full_field=True):
        super().__init__()
        self.timestep = args.model_timestep
        self.full_field = full_field
        self._open(data_folder, data_index, downsample_rate, x_range, y_range, use_patch)

    def __len__(self):
        return self.data_length // self.timestep

    def __getitem__(self, index):
        ps, vs = [], []
        for t in range(self.timestep):
            i = self.data_index[index * self.timestep + t]
            ps.append(self._load_plane(self.p_plane_files[i], self.p_norm))
            vs.append(self._load_plane(self.v_plane_files[i], self.v_norm))
        return torch.stack(ps), torch.stack(vs)


class FullFieldNSDataset(Dataset):
    """Full-field channel-flow samples for the plane-prediction observer with the physics-informed term
    (libs/pde_data_loader.py:135-198; consumer run_pde_observers.py:200-231).  Folder format: per-timestep
    `U_field_######.npy`, `W_field_######.npy` (Nx, Ny+1, Nz), `V_field_######.npy` (Nx, Ny, Nz) and a pickled `metadata.npy`
    with `re`, `U_field.dpdx[i]`, `V_field.{mean,std}` and `P_planes.{mean,std}`.

    Item: (wall plane of v, normalised [T, X, Z]; target planes of v, normalised [T, P, X, Z]; U, V, W [T, ...];
    Re [T]; dPdx [T]).  The input plane and every target plane share ONE normaliser, the statistics of the wall plane
    V[:, -1, :] (:154-161)."""

    def __init__(self, args, data_folder, data_index, plane_indexs, downsample_rate, x_range, y_range, use_patch=False,
                 full_field=True):
        super().__init__()
        self.timestep = args.model_timestep
        self.data_folder, self.full_field = data_folder, full_field
        self.downsample_rate, self.x_range, self.y_range = downsample_rate, x_range, y_range      # kept, unused (as upstream)
        self.metadata = np.load(os.path.join(data_folder, 'metadata.npy'), allow_pickle=True).tolist()
        self.re = torch.tensor(self.metadata['re'])
        self.dpdx_all = self.metadata['U_field']['dpdx']
        self.file_list = os.listdir(data_folder)
        self.u_field_files, self.v_field_files, self.w_field_files = (
            sorted(f for f in self.file_list if tag in f) for tag in ('U_field', 'V_field', 'W_field'))
        self.scale_factor = 1
        v_stats = self.metadata['V_field']
        self.bound_v_mean, self.bound_v_std = v_stats['mean'][:, -1, :], v_stats['std'][:, -1, :] / self.scale_factor
        self.v_field_mean, self.v_field_std = v_stats['mean'][:, 1:-1, :], v_stats['std'][:, 1:-1, :]
        self.data_index = data_index
        self.data_length = len(data_index)
        self.plane_indexs = plane_indexs
        self.bound_v_norm = NormalizerGivenMeanStd(self.bound_v_mean, self.bound_v_std)
        self.v_field_norm = self.bound_v_norm
        self.p_plane_mean, self.p_plane_std = self.metadata['P_planes']['mean'], self.metadata['P_planes']['std']
        self.p_plane_norm = NormalizerGivenMeanStd(self.p_plane_mean, self.p_plane_std)

    def __len__(self):
        return self.data_length // self.timestep

    def _field(self, names, i):
        return torch.tensor(np.load(os.path.join(self.data_folder, names[i])))

    def __getitem__(self, index):
        planes, targets, us, vs, ws, res, dpdxs = [], [], [], [], [], [], []
        for t in range(self.timestep):
            i = self.data_index[index * self.timestep + t]
            v = self._field(self.v_field_files, i)
            us.append(self._field(self.u_field_files, i))
            vs.append(v)
            ws.append(self._field(self.w_field_files, i))
            planes.append(self.bound_v_norm.encode(v[:, -1, :]))
            targets.append(torch.stack([self.v_field_norm.encode(v[:, p, :]) for p in self.plane_indexs]))
            res.append(self.re)
            dpdxs.append(self.dpdx_all[i])
        return (torch.stack(planes), torch.stack(targets), torch.stack(us), torch.stack(vs), torch.stack(ws),
                torch.tensor(res), torch.tensor(dpdxs))


class _ItemIndex(Dataset):
    """Index-only stand-in of a dataset of `n` items: item i is i.  A DataLoader over it visits the items in the order a
    DataLoader with the same arguments visits the dataset itself, and draws from the generator exactly as that one does."""

    def __init__(self, n):
        self.n = int(n)

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        return i


class _RankIndexBatches(object):
    """The index loader of a device-resident batch source and this rank's slice of its batches: a DataLoader with the host
    loader's arguments over an index-only dataset of `n` items, so order, draws from the generator, ragged tail and drop_last
    are the host loader's; of every global batch of batch_size * world items a rank keeps its own batch_size."""

    def _index_loader(self, n, batch_size, shuffle, generator, drop_last, rank, world):
        self.batch_size, self.rank, self.world = int(batch_size), int(rank), int(world)
        if not 0 <= self.rank < self.world:
            raise ValueError(f"{type(self).__name__}: rank {rank} outside a world of {world}")
        self.loader = DataLoader(_ItemIndex(n), batch_size=self.batch_size * self.world, shuffle=shuffle, drop_last=drop_last,
                                 generator=generator)

    def __len__(self):
        return len(self.loader)

    def index_batches(self):
        """this rank's item indices of every batch of one epoch (CPU int64), in the host loader's order"""
        for items in self.loader:
            if self.world > 1:
                n = items.shape[0]
                assert n % self.world == 0, f"global batch {n} not divisible by world size {self.world}"
                per = n // self.world
                items = items[self.rank * per:(self.rank + 1) * per]
            yield items


_TORCH_OF = {np.dtype(np.float32): torch.float32, np.dtype(np.float64): torch.float64}
_STAGE_BYTES = 64 << 20
_POOLS = weakref.WeakValueDictionary()      # (folder, device) -> _FolderPool: datasets over one folder share one pool


class _TagPool(object):
    """The files of one tag (`P_planes`, `V_field`, ...) of a folder: slot numbers are handed out when a DeviceBatches is
    built (`plan`), the files of the planned slots are read - once each - and uploaded when the first batch is asked for."""

    def __init__(self, tag):
        self.tag, self.shape, self.dtype = tag, None, None
        self.slots, self.names = {}, []      # file name -> slot, slot -> file name
        self.tensor, self.resident = None, 0

    @property
    def snap_bytes(self):
        return int(np.prod(self.shape)) * self.dtype.itemsize


class _FolderPool(object):
    def __init__(self, folder, device):
        self.folder, self.device, self.tags = folder, device, {}

    def planned_bytes(self):
        return sum(len(t.names) * t.snap_bytes for t in self.tags.values())

    def plan(self, tag, names, max_bytes):
        """Slots of the files `names` of `tag`: new files get the next slots after their headers were checked against the
        tag's shape and dtype and the whole pool against `max_bytes`.  Nothing is read or uploaded yet; no GPU is needed."""
        t = self.tags.get(tag) or _TagPool(tag)
        shape, dtype, new = t.shape, t.dtype, []
        for name in dict.fromkeys(names):
            if name in t.slots:
                continue
            head = np.load(os.path.join(self.folder, name), mmap_mode="r")
            if head.dtype not in _TORCH_OF:
                raise TypeError(f"{os.path.join(self.folder, name)}: dtype {head.dtype} (float32 or float64 files can stay on the device)")
            if shape is None:
                shape, dtype = tuple(head.shape), head.dtype
            elif (tuple(head.shape), head.dtype) != (shape, dtype):
                raise ValueError(f"{os.path.join(self.folder, name)}: shape {tuple(head.shape)} dtype {head.dtype}, but the other "
                                 f"{tag} files of the pool hold shape {shape} dtype {dtype}")
            new.append(name)
        if new:
            add = len(new) * int(np.prod(shape)) * dtype.itemsize
            have = self.planned_bytes()
            if have + add > max_bytes:
                raise MemoryError(f"device-resident data of {self.folder}: the pool would hold {have + add} bytes, the budget is "
                                  f"{int(max_bytes)} bytes (max_bytes; the host loader remains the path for such a folder)")
            t.shape, t.dtype = shape, dtype
            for name in new:
                t.slots[name] = len(t.names)
                t.names.append(name)
            self.tags[tag] = t
        return [t.slots[n] for n in names]

    def tensor(self, tag):
        """The (slots, *shape) device tensor of `tag` in the files' dtype with every planned slot resident: the missing files
        are read once and travel in chunks through one pinned staging buffer."""
        t = self.tags[tag]
        n = len(t.names)
        if t.resident == n:
            return t.tensor
        tdtype = _TORCH_OF[t.dtype]
        full = torch.empty((n,) + t.shape, dtype=tdtype, device=self.device)
        if t.resident:
            full[:t.resident].copy_(t.tensor)
        chunk = max(1, min(n - t.resident, _STAGE_BYTES // max(t.snap_bytes, 1)))
        stage = torch.empty((chunk,) + t.shape, dtype=tdtype).pin_memory()
        stream = torch.cuda.current_stream(self.device)
        for c0 in range(t.resident, n, chunk):
            m = min(chunk, n - c0)
            for k in range(m):
                a = np.load(os.path.join(self.folder, t.names[c0 + k]))
                if (tuple(a.shape), a.dtype) != (t.shape, t.dtype):
                    raise ValueError(f"{os.path.join(self.folder, t.names[c0 + k])}: shape {tuple(a.shape)} dtype {a.dtype} "
                                     f"differs from its header ({t.shape}, {t.dtype})")
                stage[k].copy_(torch.from_numpy(np.ascontiguousarray(a)))
            full[c0:c0 + m].copy_(stage[:m], non_blocking=True)
            stream.synchronize()             # the staging buffer is refilled next
        t.tensor, t.resident = full, n
        return full


def _folder_pool(folder, device):
    key = (os.path.realpath(folder), str(device))
    pool = _POOLS.get(key)
    if pool is None:
        pool = _POOLS[key] = _FolderPool(folder, device)
    return pool


class DeviceBatches(_RankIndexBatches):
    """Batches of a PDEDataset, SequentialPDEDataset or FullFieldNSDataset assembled on the GPU from a device-resident pool of
    the folder's raw files: iterating yields the tuples of float32 device tensors that
    `DevicePrefetcher(DataLoader(dataset, batch_size * world, shuffle, drop_last, generator))` followed by `shard_batch` yields,
    bit for bit (NaN signs aside: they are the processor's), without per-item host work.

    Pool: every file `dataset.data_index` references is read once, kept in its file dtype and shared by the datasets of one
    folder (train and test); shuffled gather, downsample, crop, plane select, normalisation in the host's arithmetic type and
    the cast to float32 are one functional.data_gather launch per tensor.  Order: the index batches come from a DataLoader with
    the same arguments over an index-only dataset of the same length, so order, generator consumption, ragged tail and
    drop_last are the host loader's by construction.  Data parallelism: a rank gathers only its slice of the global batch.
    `use_patch` datasets are not covered; a pool beyond `max_bytes` raises and the host loader remains the path."""

    def __init__(self, dataset, batch_size, device, shuffle, generator, drop_last=False, rank=0, world=1, max_bytes=8 << 30):
        if getattr(dataset, "use_patch", False):
            raise NotImplementedError("DeviceBatches: use_patch datasets are assembled on the host (DataLoader + DevicePrefetcher)")
        if not isinstance(dataset, (PDEDataset, SequentialPDEDataset, FullFieldNSDataset)):
            raise NotImplementedError(f"DeviceBatches: {type(dataset).__name__} (PDEDataset, SequentialPDEDataset, FullFieldNSDataset)")
        self.dataset, self.device = dataset, torch.device(device)
        self._index_loader(len(dataset), batch_size, shuffle, generator, drop_last, rank, world)
        self.T = 1 if isinstance(dataset, PDEDataset) else int(dataset.timestep)
        index = [int(i) for i in dataset.data_index][:len(dataset) * self.T]
        self.file_index = torch.tensor(index, dtype=torch.int64).reshape(len(dataset), self.T)      # file of (item, time step)
        self.pool = _folder_pool(dataset.data_folder, self.device)
        self._slots, self._stats = {}, None
        if isinstance(dataset, FullFieldNSDataset):
            lists = {"U_field": dataset.u_field_files, "V_field": dataset.v_field_files, "W_field": dataset.w_field_files}
        else:
            p_name, v_name = _plane_names(dataset.metadata)
            lists = {p_name: dataset.p_plane_files, v_name: dataset.v_plane_files}
            self._tags = (p_name, v_name)
        for tag, files in lists.items():
            slots = self.pool.plan(tag, [files[i] for i in index], max_bytes)
            self._slots[tag] = torch.tensor(slots, dtype=torch.int64).reshape(len(dataset), self.T)
        self._plan_views()

    @staticmethod
    def _crop_extent(n, d, limit):
        return len(range(0, n, d)[:limit])

    def _plan_views(self):
        ds = self.dataset
        if isinstance(ds, FullFieldNSDataset):
            Nx, Ny, Nz = self.pool.tags["V_field"].shape
            if self.pool.tags["U_field"].shape != (Nx, Ny + 1, Nz) or self.pool.tags["W_field"].shape != (Nx, Ny + 1, Nz):
                raise ValueError(f"{ds.data_folder}: U and W fields must be (Nx, Ny + 1, Nz) around V (Nx, Ny, Nz) = {(Nx, Ny, Nz)}")
            planes = []
            for p in ds.plane_indexs:      # negative plane indices are normalised here, on the host
                if not -Ny <= int(p) < Ny:
                    raise IndexError(f"plane index {p} outside the {Ny} wall-normal planes of V")
                planes.append(int(p) % Ny)
            self.planes, self.grid = planes, (Nx, Ny, Nz)
            self._norms = {"V_field": ds.bound_v_norm}
            shapes = {"V_field": (Nx, Nz)}
        else:
            d = int(ds.downsample_rate)
            self._views = {}
            for tag in self._tags:
                shape = self.pool.tags[tag].shape
                if len(shape) != 2:
                    raise ValueError(f"{ds.data_folder}: {tag} files of shape {shape} (2-D planes expected)")
                rows, cols = self._crop_extent(shape[0], d, ds.x_range), self._crop_extent(shape[1], d, ds.y_range)
                self._views[tag] = (0, d * shape[1], d, rows, cols)
            self._norms = dict(zip(self._tags, (ds.p_norm, ds.v_norm)))
            shapes = {tag: v[3:] for tag, v in self._views.items()}
        for tag, norm in self._norms.items():
            want = shapes[tag]
            if tuple(norm.mean.shape) != tuple(want) or tuple(norm.std.shape) != tuple(want) or norm.mean.dtype != norm.std.dtype \
                    or norm.mean.dtype not in (torch.float32, torch.float64):
                raise ValueError(f"{ds.data_folder}: the statistics of {tag} ({tuple(norm.mean.shape)} {norm.mean.dtype}, "
                                 f"{tuple(norm.std.shape)} {norm.std.dtype}) must be one float dtype with the planes' shape {tuple(want)}")

    def _resident(self):
        """pool tensors and, once, the statistics: cropped, contiguous, on the device in their own dtype"""
        if self._stats is None:
            self._stats = {tag: (n.mean.contiguous().to(self.device), n.std.contiguous().to(self.device), float(n.eps))
                           for tag, n in self._norms.items()}
            ds = self.dataset
            if isinstance(ds, FullFieldNSDataset):
                files = self.file_index.reshape(-1).tolist()
                self._re_row = torch.tensor([ds.re for _ in range(self.T)]).to(self.device).float()
                self._dpdx = torch.tensor([ds.dpdx_all[i] for i in files]).reshape(self.file_index.shape).to(self.device).float()
        return {tag: self.pool.tensor(tag) for tag in self._slots}

    def __iter__(self):
        from .. import functional as F
        pools = None
        for items in self.index_batches():
            if pools is None:
                pools = self._resident()
            yield (self._full_field if isinstance(self.dataset, FullFieldNSDataset) else self._planes)(F, pools, items)

    def _planes(self, F, pools, items):
        B, out = items.shape[0], []
        for tag in self._tags:
            mean, std, eps = self._stats[tag]
            view = self._views[tag]
            t = F.data_gather(pools[tag], self._slots[tag][items].reshape(-1), view, mean, std, eps)
            out.append(t.view(B, view[3], view[4], 1) if isinstance(self.dataset, PDEDataset) else t.view(B, self.T, view[3], view[4]))
        return tuple(out)

    def _full_field(self, F, pools, items):
        B, T, P = items.shape[0], self.T, len(self.planes)
        Nx, Ny, Nz = self.grid
        mean, std, eps = self._stats["V_field"]
        slots = {tag: s[items].reshape(-1) for tag, s in self._slots.items()}
        V = pools["V_field"]
        wall = F.data_gather(V, slots["V_field"], ((Ny - 1) * Nz, Ny * Nz, 1, Nx, Nz), mean, std, eps).view(B, T, Nx, Nz)
        target = torch.empty((B, T, P, Nx, Nz), dtype=torch.float32, device=self.device)
        for k, p in enumerate(self.planes):
            F.data_gather(V, slots["V_field"], (p * Nz, Ny * Nz, 1, Nx, Nz), mean, std, eps,
                          out=target.view(-1)[k * Nx * Nz:], out_stride=P * Nx * Nz)
        fields = []
        for tag, ny in (("U_field", Ny + 1), ("V_field", Ny), ("W_field", Ny + 1)):
            fields.append(F.data_gather(pools[tag], slots[tag], (0, ny * Nz, 1, Nx, ny * Nz)).view(B, T, Nx, ny, Nz))
        on_dev = items.to(self.device)
        return (wall, target, *fields, self._re_row.expand(B, T).contiguous(), self._dpdx[on_dev])
