"""libs/envs/control_env.py surface, the part the observer training loop calls: the channel-flow right-hand side and the
physics-informed loss (NSControlEnvMatlab.compute_rhs_py :429-530, pde_loss :627-633, load_state :149-180).

What the `pde_loss_weight` branch of the observer training loop needs (run_pde_observers.py:53-57, 226-231) is an object with
the grid metrics and two methods, ChannelFlowRHS; they run on the HIP engine (fno_chanflow_*), one launch per batch instead
of ~1500 slice kernels per sample.

ChannelFlowEnv is the environment itself (NSControlEnvMatlab without MATLAB, wandb or plotting): the boundary-controlled RK3
step with its fractional-step projection (:533-613), the wall-pressure observation (:196-229, :423-427), opposition control
and the rewards / scores (:186-340), on float64 GPU tensors with an optional leading batch of independent environments."""
import numpy as np
import torch

from ... import functional as F


class ChannelFlowRHS:
    """Grid metrics + compute_rhs_py / pde_loss with the reference's names and argument meaning.

    Build it from the same `.mat` initial condition the reference loads (`from_mat`, control_env.py:149-168) or from an
    analytic tanh grid (`tanh_channel`, libs/matlab_codes/main.m:13-22)."""
    default_nu = 3.076923076923077e-04      # control_env.py:26
    default_re = 178.1899                   # :27
    default_dPdx = 0.57231059E-01 ** 2      # :161

    def __init__(self, Nx, Nz, dx, dz, y, ym, yg=None, Re=-1.0, dPdx=None):
        y, ym = np.asarray(y, dtype=np.float64).reshape(-1), np.asarray(ym, dtype=np.float64).reshape(-1)
        if yg is None:
            yg = np.concatenate(([-ym[0]], ym, [2 + ym[0]]))                 # :165
        self.Re = float(Re)                     # :25 (what the optimal-observer policy conditions its observer on)
        self.nu = self.default_nu * (self.default_re / Re) if Re > 0 else self.default_nu      # :26-29
        self.dPdx = self.default_dPdx if dPdx is None else float(dPdx)
        self.Nx, self.Ny, self.Nz = int(Nx), int(y.shape[0]), int(Nz)
        self.dx, self.dz = float(np.asarray(dx).reshape(-1)[0]), float(np.asarray(dz).reshape(-1)[0])
        self.y, self.ym, self.yg = y, ym, np.asarray(yg, dtype=np.float64).reshape(-1)
        self.grid = F.ChannelGrid(self.Nx, self.Nz, self.dx, self.dz, self.y, self.ym, self.yg, self.nu)

    @classmethod
    def from_mat(cls, load_path, Re=-1.0):
        """The grid of a reference initial-condition file (x, y, z, ym; Nx = len(x) - 2, Nz = len(z) - 2)."""
        import scipy.io
        m = scipy.io.loadmat(load_path, mat_dtype=True)
        x, y, z, ym = (np.asarray(m[k], dtype=np.float64).reshape(-1) for k in ("x", "y", "z", "ym"))
        return cls(len(x) - 2, len(z) - 2, x[1] - x[0], z[1] - z[0], y, ym, Re=Re)

    @classmethod
    def tanh_channel(cls, Nx=32, Ny=130, Nz=32, Lx=2 * np.pi, Lz=2 * np.pi, stretch=2.6, Re=-1.0):
        y = 1 + np.tanh(stretch * np.linspace(-1, 1, Ny)) / np.tanh(stretch)
        return cls(Nx, Nz, Lx / Nx, Lz / Nz, y, 0.5 * (y[1:] + y[:-1]), Re=Re)

    # -- the reference's per-field signatures (fields (Nx, Ny[+1], Nz)); a leading batch dimension is accepted too
    def compute_rhs_py(self, U, V, W, dPdx=None):
        if dPdx is None:
            dPdx = self.dPdx
        if U.dim() == 3:
            return tuple(f[0] for f in F.chanflow_rhs(self.grid, U[None], V[None], W[None], dPdx))
        return F.chanflow_rhs(self.grid, U, V, W, dPdx)

    def pde_loss(self, U, Vgt, V, W, dPdx=None):
        """||Fu_gt - Fu_pred|| + ||Fv_gt - Fv_pred|| + ||Fw_gt - Fw_pred||, summed over the batch when the fields carry
        one (the loop at run_pde_observers.py:228-230 in one call).  dPdx cancels in the difference; the argument is kept
        for signature parity."""
        if U.dim() == 3:
            U, Vgt, V, W = U[None], Vgt[None], V[None], W[None]
        return F.chanflow_pde_loss(self.grid, U.float(), Vgt.float(), V.float(), W.float())


def load_state_mat(load_path):
    """x, y, z, ym, U, V, W of a `.mat` state file: the reference's shipped initial condition (padded UU, VV, WW,
    control_env.py:170-176) or one written by dump_state (U, V, W)"""
    import scipy.io
    m = scipy.io.loadmat(load_path, mat_dtype=True)
    x, y, z, ym = (np.asarray(m[k], dtype=np.float64).reshape(-1) for k in ("x", "y", "z", "ym"))
    Nx, Nz = len(x) - 2, len(z) - 2
    if "UU" in m:
        U, V, W = m["UU"][0:Nx, :, 1:Nz + 1], m["VV"][1:Nx + 1, :, 1:Nz + 1], m["WW"][1:Nx + 1, :, 0:Nz]
    else:
        U, V, W = m["U"], m["V"], m["W"]
    return x, y, z, ym, U, V, W


def dump_state_mat(save_path, x, y, z, ym, U, V, W):
    """the keys NSControlEnvMatlab.dump_state writes (:134-147)"""
    import scipy.io
    x, z = np.asarray(x, dtype=np.float64).reshape(-1), np.asarray(z, dtype=np.float64).reshape(-1)
    scipy.io.savemat(save_path, {"x": x, "y": np.asarray(y), "z": z, "xm": 0.5 * (x[1:] + x[:-1]), "ym": np.asarray(ym),
                                 "zm": 0.5 * (z[1:] + z[:-1]), "U": np.asarray(U), "V": np.asarray(V), "W": np.asarray(W)})


class ChannelFlowEnv(ChannelFlowRHS):
    """NSControlEnvMatlab's stepping surface on the engine.  State U, W (B, Nx, Ny+1, Nz), V (B, Nx, Ny, Nz), float64 on
    `device`; a state given without the batch dimension makes B = 1 and every per-field result drops it again.  Per-sample
    scalars (dPdx, meanU0) are device tensors; `step_rk3` copies nothing to the host, `step` one (B, 13) block for `info` (the twelve diagnostics and dPdx)."""
    INFO_KEYS = ("drag_reduction/1_shear_stress", "drag_reduction/2_1_mass_flow", "drag_reduction/2_2_v_velocity",
                 "drag_reduction/2_3_w_velocity", "drag_reduction/3_1_pressure_mean",
                 "drag_reduction/3_2_dPdx_finite_difference", "drag_reduction/3_3_dPdx_reverse_cal",
                 "drag_reduction/4_1_-|divergence|", "drag_reduction/4_4_speed_norm")
    INIT_ONLY_KEY = "drag_reduction/4_2_-|now - unnoised| ÷ ｜now|"      # fill_info_init (:114) carries it, step does not

    def __init__(self, Nx, Nz, dx, dz, y, ym, U, V, W, yg=None, Re=-1.0, dPdx=None, dt=0.001, detect_plane=10, device="cuda",
                 graph=False, x=None, z=None):
        super().__init__(Nx, Nz, dx, dz, y, ym, yg=yg, Re=Re, dPdx=dPdx)
        device = torch.device(device)
        if device.type != "cuda" or not torch.cuda.is_available():
            raise RuntimeError(f"fnoengine ChannelFlowEnv: the environment steps on the GPU (got device {device}); "
                               "the engine has no CPU path")
        self.device, self.dt, self.detect_plane = device, float(dt), int(detect_plane)
        self.x, self.z = x, z
        self.poisson = F.ChannelPoisson(self.grid)
        self._graph_wanted, self._graph = bool(graph), None
        self._set_state(U, V, W)
        self.dPdx_dev = torch.full((self.B,), self.dPdx, dtype=torch.float64, device=device)
        self.ws = F.chanflow_step_workspace(self.grid, self.B, device)
        self.U_gt, self.V_gt, self.W_gt = self.U.clone(), self.V.clone(), self.W.clone()
        self.meanU0 = self._diag()[:, 8].clone()
        self.info_init = self.fill_info_init()

    # the reference keeps dPdx as a host float that every step updates; here the value lives on the device (dPdx_dev) and this
    # is its host view: reading it is a device-to-host copy, so nothing on the stepping path does.  One environment: a float,
    # as in the reference; an ensemble (B > 1, which the reference does not have): a numpy array with one value per sample
    @property
    def dPdx(self):
        if getattr(self, "dPdx_dev", None) is None:
            return self._dPdx0
        v = self.dPdx_dev.cpu()
        return float(v[0]) if self._squeeze else v.numpy()

    @dPdx.setter
    def dPdx(self, value):
        if getattr(self, "dPdx_dev", None) is None:
            self._dPdx0 = float(value)
        else:
            self.dPdx_dev.copy_(torch.as_tensor(value, dtype=torch.float64).reshape(-1).expand(self.B))

    def compute_rhs_py(self, U, V, W, dPdx=None):
        """dPdx=None means the environment's current value(s).  With an ensemble (B > 1) that is one value per sample, so the
        fields must then carry the environment's batch; any other shape has no defined pressure gradient and is refused."""
        if dPdx is None:
            if self.B == 1:
                dPdx = float(self.dPdx_dev[0])
            elif U.dim() == 4 and U.shape[0] == self.B:
                dPdx = self.dPdx_dev
            else:
                raise RuntimeError(f"ChannelFlowEnv.compute_rhs_py: dPdx=None with an ensemble of {self.B} needs fields with that "
                                   f"leading batch (got {tuple(U.shape)}); pass dPdx explicitly")
        return super().compute_rhs_py(U, V, W, dPdx)

    # -- construction -------------------------------------------------------------------------------------------------------
    @classmethod
    def from_mat(cls, load_path, **kw):
        x, y, z, ym, U, V, W = load_state_mat(load_path)
        return cls(len(x) - 2, len(z) - 2, x[1] - x[0], z[1] - z[0], y, ym, U, V, W, x=x, z=z, **kw)

    def _set_state(self, U, V, W):
        t = [torch.as_tensor(np.asarray(a.detach().cpu() if torch.is_tensor(a) else a, dtype=np.float64)) for a in (U, V, W)]
        self._squeeze = t[0].dim() == 3
        if self._squeeze:
            t = [a[None] for a in t]
        self.U, self.V, self.W = (a.to(self.device).contiguous() for a in t)
        self.B = self.U.shape[0]
        self.grid._check_fields(self.U, self.V, self.W, "ChannelFlowEnv")
        self._graph = None

    def load_state(self, load_path):
        """the fields of a `.mat` file written by dump_state or shipped with the reference (same keys)"""
        U, V, W = load_state_mat(load_path)[4:]
        self._set_state(U, V, W)

    def dump_state(self, save_path):
        x = self.dx * np.arange(self.Nx + 2) if self.x is None else self.x
        z = self.dz * np.arange(self.Nz + 2) if self.z is None else self.z
        dump_state_mat(save_path, x, self.y, z, self.ym, *(self._out(t).cpu().numpy() for t in (self.U, self.V, self.W)))

    def _out(self, t):
        return t[0] if self._squeeze else t

    def _in(self, t, shape):
        t = torch.as_tensor(t, dtype=torch.float64).to(self.device)
        return t.reshape(shape).contiguous()

    # -- the step -----------------------------------------------------------------------------------------------------------
    def step_rk3(self, opV1, opV2):
        shp = (self.B, self.Nx, self.Nz)
        v1, v2 = self._in(opV1, shp), self._in(opV2, shp)
        if self._graph_wanted:
            if self._graph is None:
                self._graph = F.GraphedChannelStep(self.grid, self.poisson, self.U, self.V, self.W, self.dPdx_dev, self.meanU0, self.dt)
                self.U, self.V, self.W, self.dPdx_dev = self._graph.U, self._graph.V, self._graph.W, self._graph.dPdx
            self._graph.opV1.copy_(v1)
            self._graph.opV2.copy_(v2)
            self._p = tuple(p.clone() for p in self._graph.step())      # the graph overwrites its own buffers next step
        else:
            F.chanflow_rk3_step(self.grid, self.poisson, self.U, self.V, self.W, v1, v2, self.dPdx_dev, self.meanU0, self.dt, ws=self.ws)
            self._p = None

    def get_boundary_pressures(self):
        p1, p2 = F.chanflow_wall_pressure(self.grid, self.poisson, self.U, self.V, self.W, self.dPdx_dev, ws=self.ws)
        return self._out(p1), self._out(p2)

    def cal_pressure(self, full=True):
        """P (Nx, Ny-1, Nz), the observation function's full field; full=False: the two wall observations only"""
        if not full:
            return self.get_boundary_pressures()
        self.P = self._out(F.chanflow_wall_pressure(self.grid, self.poisson, self.U, self.V, self.W, self.dPdx_dev, full=True, ws=self.ws)[2])
        return self.P

    def _diag(self, p2=None):
        return F.chanflow_diagnostics(self.grid, self.poisson, self.U, self.V, self.W, p2)

    def _info(self, d):
        """one dict per sample from the host copy of the diagnostics block and dPdx"""
        out = []
        for b in range(self.B):
            r = d[b]
            vals = (r[7], r[8], r[2], r[3], r[9], r[10], r[12], max(-abs(r[0]), -100.0), r[4] + r[5] + r[6])
            out.append(dict(zip(self.INFO_KEYS, (float(v) for v in vals))))
        return out

    def _host_block(self, p2):
        p2b = p2[None] if self._squeeze else p2
        return torch.cat([self._diag(p2b), self.dPdx_dev[:, None]], dim=1).cpu().numpy()      # the one device-to-host copy

    def fill_info_init(self):
        _, p2 = self.get_boundary_pressures()
        infos = self._info(self._host_block(p2))
        gt = self.reward_gt()
        for b, info in enumerate(infos):
            info[self.INIT_ONLY_KEY] = float(np.atleast_1d(gt)[b])
        return infos[0] if self._squeeze else infos

    def step(self, opV1, opV2):
        """(p2, div, done, info) of NSControlEnvMatlab.step (:639-664); with a batch, div is a list and info a list of dicts"""
        self.step_rk3(opV1, opV2)
        p2 = self._out(self._p[1]) if self._p is not None else self.get_boundary_pressures()[1]
        infos = self._info(self._host_block(p2))
        if self.info_init is not None:
            inits = [self.info_init] if self._squeeze else self.info_init
            for info, init in zip(infos, inits):
                info.update(self.cal_relative_info(info, init))
        divs = [i["drag_reduction/4_1_-|divergence|"] for i in infos]
        return (p2, divs[0], False, infos[0]) if self._squeeze else (p2, divs, False, infos)

    def cal_relative_info(self, info, init=None):
        init = self.info_init if init is None else init
        if init is None:
            raise RuntimeError("ChannelFlowEnv.cal_relative_info: info_init was reset (reset_init) and not filled again")
        return {k.replace("drag_reduction", "drag_reduction_relative"): info[k] / init[k] for k in info if "divergence" not in k}

    def reset_init(self):
        self.info_init = None

    # -- controls, rewards and scores (each reads the diagnostics block or a field slice) -----------------------------------
    def gt_control(self):
        return self._out(-self.V[:, :, self.detect_plane, :]).clone(), self._out(-self.V[:, :, -self.detect_plane, :]).clone()

    def rand_control(self, P):
        raise NotImplementedError("rand_control is a MATLAB call (compute_opposition) in the reference; it is not on this path")

    def vis_state(self, *a, **kw):
        raise NotImplementedError("visualisation is outside the engine's path")

    def _scalar(self, col):
        v = self._diag()[:, col].cpu()
        return float(v[0]) if self._squeeze else v.numpy()

    def cal_div(self):
        """the divergence field (Nx, Ny-1, Nz) (:186-194), a slice expression on the device"""
        U, V, W = self.U, self.V, self.W
        hy = torch.as_tensor(np.diff(self.y), device=self.device)[None, None, :, None]
        d = (torch.roll(U, -1, 1) - U)[:, :, 1:-1] / self.dx + (V[:, :, 1:] - V[:, :, :-1]) / hy + \
            (torch.roll(W, -1, 3) - W)[:, :, 1:-1] / self.dz
        return self._out(d)

    def reward_div(self, bound=-100):
        r = -np.abs(self._scalar(0))
        return max(r, bound) if self._squeeze else np.maximum(r, bound)

    def _rel_reward(self, ref, bound):
        r = 0
        for a, b in zip(ref, (self.U, self.V, self.W)):
            a = a.to(self.device).reshape(b.shape)
            num, den = (a - b).flatten(1).norm(dim=1), a.flatten(1).norm(dim=1)
            r = r - torch.where(den > 0, num / den.clamp_min(1e-300), torch.zeros_like(num)).cpu().numpy()
        r = np.maximum(r, bound)
        return float(r[0]) if self._squeeze else r

    def reward_gt(self, bound=-100):
        return self._rel_reward((self.U_gt, self.V_gt, self.W_gt), bound)

    def reward_td(self, prev_U, prev_V, prev_W, bound=-100):
        return self._rel_reward(tuple(torch.as_tensor(p, dtype=torch.float64) for p in (prev_U, prev_V, prev_W)), bound)

    def cal_bulk_v(self):
        return self._scalar(8)

    def cal_velocity_mean(self, velocity_name="U", sample_index=10):
        if velocity_name not in ("U", "V", "W"):
            raise RuntimeError("not supported velocity!")
        if sample_index is None:
            return self._scalar({"U": 1, "V": 2, "W": 3}[velocity_name])
        v = getattr(self, velocity_name).abs()[:, :, -sample_index:, :].mean(dim=(1, 2, 3)).cpu()
        return float(v[0]) if self._squeeze else v.numpy()

    def cal_speed_norm(self):
        d = self._diag()[:, 4:7].sum(dim=1).cpu()
        return float(d[0]) if self._squeeze else d.numpy()

    def cal_dudy(self):
        hy = np.diff(self.y)
        return [self._out((self.U[:, :, j + 1, :] - self.U[:, :, j, :]) / hy[j]) for j in range(self.Ny - 1)]

    def cal_shear_stress(self):
        return self._scalar(7)

    def cal_dpdx_finite_difference(self, pressure_top):
        p = self._in(pressure_top, (self.B, self.Nx, self.Nz))
        v = ((p[:, 1:] - p[:, :-1]) / self.dx).abs().mean(dim=2).mean(dim=1).abs().cpu()
        return float(v[0]) if self._squeeze else v.numpy()

    def add_random_noise(self, noise_scale, overwrite=False):
        for t in (self.U, self.V, self.W):
            n = torch.randn(t.shape, dtype=torch.float64, device=self.device) * noise_scale
            if overwrite:
                t.copy_(n)
            else:
                t.add_(n)
