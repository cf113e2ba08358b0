"""NSControlEnv2D on the engine: the reference's second control environment (libs/envs/ns_control_2d.py), the "python env" of
configs/python_env_rno.yaml: a 41 x 41 channel, periodic in x, with wall blowing and suction, float64.

The state of `ensemble` = B environments is (B, ny, nx) device tensors; one workgroup steps one environment with its whole state
in LDS (csrc/k_ns2d.h), so a Reynolds-number or forcing sweep is one launch.  `step` makes at most three engine launches (the
capped solve, the fixed-mass bisection, the diagnostics) and one device-to-host copy of 16 doubles per environment.  Around
them it issues a few elementwise torch kernels on (B,) or (B, nx) tensors: 3 * F for the bracket, copies of the bisected force,
of the first bulk velocity and of the returned pressure row, and the caller's gt_control negation.  `cal_bulk_v` / `reset_init`
launch the solve kernel for zero steps to get mean|u| in that kernel's summation order.  There is no CPU path.  With B = 1 every result drops the batch dimension and `info` is a dict, as the reference; with B > 1, `div` is a list and
`info` a list of dicts, as ChannelFlowEnv.step.

Additions to the reference's surface, so that run_control's loop shape works on both environments: `step(opV1, opV2)` beside
`step(bc)`, and `get_boundary_pressures()` -> (p[0, :], p[-1, :]).  `print_info` defaults to False.  get_state / set_state
carry no `v_scale` (the reference's get_state raises AttributeError on it).  What needs MATLAB or wandb (vis_state,
plot_spatial_distribution, cal_dpdx_reverse) and what reads attributes the reference class never defines (reward_gt, reward_td)
raises NotImplementedError."""
import numpy as np
import torch

from ... import functional as F


class NSControlEnv2D:
    INFO_KEYS = F.NS2D_DIAG
    _REP = len(F.NS2D_SOLVE_OUT) + len(F.NS2D_FIXED_OUT) + len(F.NS2D_DIAG)

    def __init__(self, args, detect_plane, bc_type, ensemble=1, device="cuda", init_v=None):
        device = torch.device(device)
        if device.type != "cuda" or not torch.cuda.is_available():
            raise RuntimeError(f"fnoengine NSControlEnv2D: the environment steps on the GPU (got device {device}); "
                               "the engine has no CPU path")
        self.device = device
        self.detect_plane = detect_plane
        self.bc_type = bc_type
        self.fix_flow = bool(args.fix_flow)
        self.B = B = max(int(ensemble), 1)
        self._squeeze = B == 1

        # initialize system states (:78-95)
        if init_v is not None:
            init_v = np.asarray(init_v, dtype=np.float64)
            self.ny, self.nx = init_v.shape[-2:]
        else:
            self.nx, self.ny = 41, 41
        self.nt, self.nit, self.c = 10, 50, 1
        self.dx, self.dy = 2 / (self.nx - 1), 2 / (self.ny - 1)
        self.x, self.y = np.linspace(0, 2, self.nx), np.linspace(0, 2, self.ny)
        self.X, self.Y = np.meshgrid(self.x, self.y)
        self.rho, self.dt = 1, .01
        self.u_scale, self.v_scale_main, self.v_scale_noise = 1.0, 0.15, 0.1
        self.step_cap = 5000

        # initial conditions (:99-104): the one host draw of the reference, shared by the ensemble
        if init_v is None:
            init_v = np.ones((self.ny, self.nx)) * self.v_scale_main + np.random.rand(self.ny, self.nx) * self.v_scale_noise
        v = np.broadcast_to(init_v, (B, self.ny, self.nx))
        self.v = torch.from_numpy(np.array(v, order="C")).to(device)
        self.u = torch.full((B, self.ny, self.nx), self.u_scale, dtype=torch.float64, device=device)
        self.p = self.v.clone()
        self.un, self.vn = torch.empty_like(self.u), torch.empty_like(self.v)
        self.Re = args.Re
        self._nu = self._per_env(self.u_scale / np.asarray(args.Re, dtype=np.float64), "Re")
        self._F = self._per_env(getattr(args, "F", 4.0), "F")
        self._rep = torch.zeros(B * self._REP, dtype=torch.float64, device=device)
        self._zero = torch.zeros(B, dtype=torch.float64, device=device)
        self._max_f = torch.empty(B, dtype=torch.float64, device=device)
        self._ptop = torch.empty((B, self.nx), dtype=torch.float64, device=device)
        self.bulk_v = self.solve(None, -1, self.p, self.u, self.v, self.dx, self.dy, self.dt, self.rho, self._nu, self._F,
                                 update_state=True)
        self.init_bulk_v = None
        self.info_init = None

    # -- plumbing ----------------------------------------------------------------------------------------------------------
    def _grid(self, dx=None, dy=None, dt=None, rho=None):
        return F.Ns2dGrid(self.nx, self.ny, self.nit, self.dx if dx is None else dx, self.dy if dy is None else dy,
                          self.dt if dt is None else dt, self.rho if rho is None else rho)

    def _per_env(self, value, name):
        if torch.is_tensor(value):
            t = value.to(self.device, torch.float64).reshape(-1)
        else:
            t = torch.from_numpy(np.asarray(value, dtype=np.float64).reshape(-1)).to(self.device)
        if t.numel() == 1:
            t = t.repeat(self.B)
        if t.numel() != self.B:
            raise RuntimeError(f"fnoengine NSControlEnv2D: `{name}` must be a scalar or have one entry per environment ({self.B}), got {t.numel()}")
        return t.contiguous()

    def _out(self, t):
        """device tensor -> what the caller sees: B = 1 drops the batch dimension"""
        return t[0] if self._squeeze else t

    def _host(self, t):
        a = t.detach().cpu().numpy()
        return float(a[0]) if self._squeeze else a

    def _field(self, t, name):
        t = torch.as_tensor(t, dtype=torch.float64).to(self.device)
        if t.dim() == 2:
            t = t[None]
        if tuple(t.shape) != (self.B, self.ny, self.nx):
            raise RuntimeError(f"fnoengine NSControlEnv2D: `{name}` must be ({self.B}, {self.ny}, {self.nx}) (got {tuple(t.shape)})")
        return t

    def _wall(self, w, name):
        if torch.is_tensor(w) or isinstance(w, np.ndarray) or np.ndim(w) > 0:
            t = torch.as_tensor(w, dtype=torch.float64).to(self.device)
            if t.dim() == 0:
                t = t.reshape(1, 1)
            elif t.dim() == 1:
                if t.numel() != self.nx:
                    raise RuntimeError(f"fnoengine NSControlEnv2D: `{name}` must have nx = {self.nx} entries (got {t.numel()})")
                t = t[None]
            if t.dim() != 2 or t.shape[1] not in (1, self.nx) or t.shape[0] not in (1, self.B):
                raise RuntimeError(f"fnoengine NSControlEnv2D: `{name}` must be a scalar, ({self.nx},) or ({self.B}, {self.nx}) (got {tuple(t.shape)})")
            return t.expand(self.B, self.nx).contiguous()
        return torch.full((self.B, self.nx), float(w), dtype=torch.float64, device=self.device)

    def _bc(self, bc):
        if bc is None:
            return None, None
        return self._wall(bc[0], "bc[0]"), self._wall(bc[1], "bc[1]")

    def _views(self):
        B, n = self.B, (len(F.NS2D_SOLVE_OUT), len(F.NS2D_FIXED_OUT), len(F.NS2D_DIAG))
        r, at = self._rep, [0, B * n[0], B * (n[0] + n[1]), B * self._REP]
        return [r[at[k]:at[k + 1]].view(B, n[k]) for k in range(3)]

    @property
    def nu(self):
        return self._host(self._nu)

    @nu.setter
    def nu(self, value):
        self._nu = self._per_env(value, "nu")

    @property
    def F(self):
        return self._host(self._F)

    @F.setter
    def F(self, value):
        self._F = self._per_env(value, "F")

    # -- state management ----------------------------------------------------------------------------------------------------
    def get_state(self):
        host = lambda t: self._out(t).detach().cpu().numpy().copy()
        return {'nx': self.nx, 'ny': self.ny, 'nt': self.nt, 'nit': self.nit, 'c': self.c, 'dx': self.dx, 'dy': self.dy,
                'x': self.x, 'y': self.y, 'X': self.X, 'Y': self.Y, 'rho': self.rho, 'nu': self.nu, 'F': self.F, 'dt': self.dt,
                'u': host(self.u), 'un': host(self.un), 'v': host(self.v), 'vn': host(self.vn), 'p': host(self.p)}

    def set_state(self, state):
        for k in ('nx', 'ny', 'nt', 'nit', 'c', 'dx', 'dy', 'x', 'y', 'X', 'Y', 'rho', 'dt'):
            setattr(self, k, state[k])
        self.nu, self.F = state['nu'], state['F']
        for k in ('u', 'un', 'v', 'vn', 'p'):
            setattr(self, k, self._field(state[k], k).clone().contiguous())
        self._ptop = torch.empty((self.B, self.nx), dtype=torch.float64, device=self.device)

    # -- scores --------------------------------------------------------------------------------------------------------------
    def _diag(self):
        out, _ = F.ns2d_diagnostics(self._grid(), self.p, self.u, self.v, self._nu)
        return out

    def cal_bulk_v(self):
        return self._host(self._bulk_v_dev())

    def _bulk_v_dev(self):
        """mean|u| in the solve kernel's own summation order: a launch that takes no step (udiff starts at 1.0)"""
        out = F.ns2d_solve(self._grid(), self.p, self.u, self.v, self._F, self._nu, u_diff_thre=2.0, update_state=False)
        return out[:, 0].clone()

    def cal_div(self):
        u, v = self.u, self.v
        return self._host((u[:, 10, 10] - u[:, 9, 10]) / self.dx + (v[:, 10, 10] - v[:, 10, 9]) / self.dy)

    def cal_pressure(self):
        return self._out(self.p)

    def cal_velocity_mean(self, velocity_name='U', sample_index=10):
        if velocity_name == 'U':
            a = self.u
        elif velocity_name == 'V':
            a = self.v
        else:
            raise RuntimeError("not supported velocity!")
        if sample_index is not None:
            return self._host(a.abs()[:, -sample_index, :].mean(dim=1))
        return self._host(self._diag()[:, 1 if velocity_name == 'U' else 2])

    def cal_speed_norm(self):
        return self._host(self._diag()[:, 6])

    def cal_dudy(self):
        return [self._out((self.u[:, i + 1, :] - self.u[:, i, :]) / self.dy) for i in range(self.ny - 2)]

    def cal_shear_stress(self):
        return self._host(self._diag()[:, 0])

    def reward_div(self, bound=-100):
        r = -np.abs(self.cal_div())
        return max(r, bound) if self._squeeze else np.maximum(r, bound)

    def cal_relative_info(self, info):
        """the first info becomes the reference and yields {} (:249-258); a list of infos (an ensemble) gives a list"""
        many = isinstance(info, (list, tuple))
        infos = list(info) if many else [info]
        if self.info_init is None:
            self.info_init = [dict(i) for i in infos]
            out = [{} for _ in infos]
        else:
            out = [{k.replace("drag_reduction", "drag_reduction_relative"): i[k] / (init[k] + 1e-9) for k in i}
                   for i, init in zip(infos, self.info_init)]
        return out if many else out[0]

    def _unsupported(self, what, why):
        raise NotImplementedError(f"fnoengine NSControlEnv2D.{what}: {why}")

    def cal_dpdx_reverse(self, layer_index=-1):
        self._unsupported("cal_dpdx_reverse", "the reference calls MATLAB (compute_dpdx_reverse) on 3-D fields this environment does not have")

    def reward_gt(self, bound=-100):
        self._unsupported("reward_gt", "reads U_gt, V_gt, W_gt, which the reference class never defines")

    def reward_td(self, prev_U, prev_V, prev_W, bound=-100):
        self._unsupported("reward_td", "reads U, V, W, which the reference class never defines")

    def vis_state(self, *a, **k):
        self._unsupported("vis_state", "plotting is out of scope")

    def plot_spatial_distribution(self, step_index):
        self._unsupported("plot_spatial_distribution", "needs MATLAB and wandb")

    # -- control policies ----------------------------------------------------------------------------------------------------
    def rand_control(self):
        bc = self.gt_control()
        scale = torch.from_numpy(np.random.rand(self.B) * 3).to(self.device)
        bc[1] = self._out(-self.v[:, -10, :] * scale[:, None])
        bc[0] = 0
        return bc

    def gt_control(self, lower_zero=True, minus_mean=False):
        """opposition control (:346-357): row -10 is hard-coded in the reference, `detect_plane` is stored and unused"""
        top, low = -self.v[:, -10, :], -self.v[:, 10, :]
        if minus_mean:
            top, low = top - top.mean(dim=1, keepdim=True), low - low.mean(dim=1, keepdim=True)
        return [0 if lower_zero else self._out(low), self._out(top)]

    # -- solver ----------------------------------------------------------------------------------------------------------------
    def _raise_on_cap(self, hit):
        if hit:
            raise RuntimeError("Not converged solving!")

    def solve(self, bc, max_step, p_copy, u_copy, v_copy, dx, dy, dt, rho, nu, F_, update_state, u_diff_thre=1e-2):
        """NSControlEnv2D.solve (:359-491) on the engine from the given fields; returns bulk_v (per environment with B > 1)"""
        p, u, v = (self._field(t, n).clone() for t, n in ((p_copy, "p_copy"), (u_copy, "u_copy"), (v_copy, "v_copy")))
        nu, F_ = self._per_env(nu, "nu"), self._per_env(F_, "F")
        lo, hi = self._bc(bc)
        un, vn = (torch.empty_like(u), torch.empty_like(v)) if update_state else (None, None)
        out = F.ns2d_solve(self._grid(dx, dy, dt, rho), p, u, v, F_, nu, lo, hi, max_step=max_step, u_diff_thre=u_diff_thre,
                           step_cap=self.step_cap, update_state=update_state, un=un, vn=vn)
        host = out.cpu().numpy()
        self.last_steps = host[:, 1].astype(np.int64)
        self._raise_on_cap((host[:, 2] == F.NS2D_STATUS.index("cap")).any())
        if update_state:
            self.un, self.vn, self.p, self.u, self.v = un, vn, p, u, v
            self.dx, self.dy, self.dt, self.rho = dx, dy, dt, rho
            self._nu, self._F = nu, F_
        return float(host[0, 0]) if self._squeeze else host[:, 0].copy()

    def solve_fixed_mass(self, bc, target_flow, min_f=0.0, max_f=3.0, max_step=500, error_threshold=1e-4, verbose=True,
                         return_overflow=True):
        """solve_fixed_mass (:493-536) in one launch; the state is not changed.  Returns (result_f, flow, error)."""
        lo, hi = self._bc(bc)
        out = F.ns2d_fixed_mass(self._grid(), self.p, self.u, self.v, self._F, self._nu, self._per_env(target_flow, "target_flow"),
                                self._per_env(min_f, "min_f"), self._per_env(max_f, "max_f"), lo, hi, step_cap=self.step_cap,
                                max_bisect=max_step, error_threshold=error_threshold)
        host = out.cpu().numpy()
        self.last_fixed = host
        self._raise_on_cap((host[:, 5] == F.NS2D_FIXED_STATUS.index("cap")).any())
        if not return_overflow:
            assert not (host[:, 5] == F.NS2D_FIXED_STATUS.index("overflow")).any(), "flow outside the bracket of min_f and max_f"
        if verbose:
            print(f"Solve step: {host[:, 3]}, target: {target_flow}, result flow: {host[:, 1]}, force: {host[:, 0]}, error: {host[:, 2]}")
        return tuple(float(host[0, k]) if self._squeeze else host[:, k].copy() for k in range(3))

    def get_top_pressure(self, extend_to_2d=True):
        return self._out(self.p[:, -1, :])

    def get_boundary_pressures(self):
        """(p[0, :], p[-1, :]): an addition to the reference's surface, so that run_control's loop reads both environments alike"""
        return self._out(self.p[:, 0, :]), self._out(self.p[:, -1, :])

    def reset_init(self):
        self.init_bulk_v = self._bulk_v_dev()
        self.info_init = None

    def step(self, bc, opV2=None, print_info=False):
        """(pressure_top, div, done, info) of NSControlEnv2D.step (:546-586).  `step(bc)` as the reference, or
        `step(opV1, opV2)` (an addition).  At most three engine launches and one device-to-host copy (small elementwise torch
        kernels beside them: see the module's docstring)."""
        if isinstance(opV2, bool):
            opV2, print_info = None, opV2
        if opV2 is not None:
            bc = (bc, opV2)
        lo, hi = self._bc(bc)
        g = self._grid()
        rs, rf, rd = self._views()
        F.ns2d_solve(g, self.p, self.u, self.v, self._F, self._nu, lo, hi, max_step=3, step_cap=self.step_cap, update_state=True,
                     un=self.un, vn=self.vn, out=rs)
        if self.init_bulk_v is None:                       # reset_init (:542-544): mean|u| of the new state
            self.init_bulk_v = rs[:, 0].clone()
            self.info_init = None
        if self.fix_flow:
            torch.mul(self._F, 3.0, out=self._max_f)
            F.ns2d_fixed_mass(g, self.p, self.u, self.v, self._F, self._nu, self.init_bulk_v, self._zero, self._max_f, lo, hi,
                              step_cap=self.step_cap, out=rf)
            self._F = rf[:, 0].clone()
        F.ns2d_diagnostics(g, self.p, self.u, self.v, self._nu, dpdx=self._F if self.fix_flow else None, out=rd, ptop=self._ptop)
        host = self._rep.cpu().numpy()                     # the one device-to-host copy
        B, n0, n1 = self.B, len(F.NS2D_SOLVE_OUT), len(F.NS2D_FIXED_OUT)
        hs, hf, hd = host[:B * n0].reshape(B, n0), host[B * n0:B * (n0 + n1)].reshape(B, n1), host[B * (n0 + n1):].reshape(B, -1)
        self.last_steps, self.last_fixed = hs[:, 1].astype(np.int64), (hf.copy() if self.fix_flow else None)
        self._raise_on_cap((hs[:, 2] == F.NS2D_STATUS.index("cap")).any() or
                           (self.fix_flow and (hf[:, 5] == F.NS2D_FIXED_STATUS.index("cap")).any()))
        infos = [dict(zip(self.INFO_KEYS, (float(x) for x in row))) for row in hd]
        if np.isnan(hd[:, 6]).any():
            print("control exploded!")
        for info, rel in zip(infos, self.cal_relative_info(infos)):
            info.update(rel)
        if print_info:
            print(infos[0] if self._squeeze else infos)
        divs = [i["drag_reduction/4_1_-|divergence|"] for i in infos]
        ptop = self._ptop.clone()
        return (ptop[0], divs[0], False, infos[0]) if self._squeeze else (ptop, divs, False, infos)
