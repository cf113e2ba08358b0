"""The 3-D channel-flow solver (fp64): grid, wall-pressure Poisson operator, RK3 step, projection, diagnostics, graph capture.
"""
import ctypes as C

import torch

from .. import _lib
from ._core import _bytes, _call, _operand, _per_sample, _refuse, _require_cuda, STREAM


# ----------------------------------------------------------------------------
# channel-flow RHS and the physics-informed loss (libs/envs/control_env.py:429-530, 627-633)
# ----------------------------------------------------------------------------
class ChannelGrid:
    """The staggered channel grid the kernels need: sizes, uniform spacings dx, dz, viscosity nu and the wall-normal
    metrics y (Ny faces), ym (Ny-1 centres), yg (Ny+1 ghost-extended centres).  Packs the reciprocal spacings once on the
    host (fno_chanflow_pack_metrics) and keeps one device copy per GPU."""

    def __init__(self, Nx, Nz, dx, dz, y, ym, yg, nu):
        import numpy as np
        y, ym, yg = (np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(-1)) for a in (y, ym, yg))
        self.Nx, self.Ny, self.Nz = int(Nx), int(y.shape[0]), int(Nz)
        if ym.shape[0] != self.Ny - 1 or yg.shape[0] != self.Ny + 1:
            raise ValueError(f"channel grid: y has {self.Ny} faces, so ym needs {self.Ny - 1} and yg {self.Ny + 1} entries "
                             f"(got {ym.shape[0]}, {yg.shape[0]})")
        self.dx, self.dz, self.nu = float(dx), float(dz), float(nu)
        self.y, self.ym, self.yg = y, ym, yg
        self._packed = None
        self._dev = {}

    def desc(self):
        return _lib.FnoChanflowGrid(self.Nx, self.Ny, self.Nz, self.dx, self.dz, self.nu)

    def metrics(self, device):
        import numpy as np
        if self._packed is None:
            packed = np.zeros(3 * (self.Ny + 2), dtype=np.float64)
            dp = C.POINTER(C.c_double)
            _lib.check(_lib.lib().fno_chanflow_pack_metrics(self.Ny, self.y.ctypes.data_as(dp), self.ym.ctypes.data_as(dp),
                                                            self.yg.ctypes.data_as(dp), packed.ctypes.data_as(dp)),
                       "chanflow_pack_metrics")
            self._packed = packed
        if device not in self._dev:
            self._dev[device] = torch.from_numpy(self._packed).to(device)
        return self._dev[device]

    def __getstate__(self):
        st = dict(self.__dict__)
        st["_dev"] = {}
        return st

    def _check_fields(self, U, V, W, who):
        B = U.shape[0]
        su, sv = (B, self.Nx, self.Ny + 1, self.Nz), (B, self.Nx, self.Ny, self.Nz)
        if tuple(U.shape) != su or tuple(W.shape) != su or tuple(V.shape) != sv:
            raise RuntimeError(f"fnoengine {who}: expected U, W {su} and V {sv}, got {tuple(U.shape)}, {tuple(W.shape)}, "
                               f"{tuple(V.shape)}")
        for t, n in ((U, "U"), (V, "V"), (W, "W")):
            if not t.is_cuda:
                raise RuntimeError(f"fnoengine {who}: `{n}` must live on the GPU (got {t.device}); the engine has no CPU path")


def chanflow_rhs(grid, U, V, W, dPdx):
    """Fu, Fv, Fw = NSControlEnvMatlab.compute_rhs_py(U, V, W, dPdx) (libs/envs/control_env.py:429-530) for a batch of
    fields: U, W (B, Nx, Ny+1, Nz), V (B, Nx, Ny, Nz), fp32 or fp64; dPdx a float or a (B,) tensor.  Not differentiable
    (the reference uses it under autograd only through pde_loss -> chanflow_pde_loss)."""
    e = "chanflow_rhs"
    grid._check_fields(U, V, W, e)
    if U.dtype not in (torch.float32, torch.float64):
        raise RuntimeError(f"fnoengine {e}: U, V, W must share one dtype, float32 or float64")
    U, V, W = (_operand(e, n, t, U, dtype=U.dtype) for n, t in (("U", U), ("V", V), ("W", W)))
    B = U.shape[0]
    dp, dflt = None, 0.0
    if torch.is_tensor(dPdx) and (dPdx.numel() > 1 or (dPdx.is_cuda and B == 1)):      # a device value is read on the device
        dp = _operand(e, "dPdx", dPdx.to(device=U.device, dtype=U.dtype), U, dtype=U.dtype, numel=B).reshape(B)
    else:
        dflt = float(dPdx)
    Fu, Fv, Fw = torch.empty_like(U), torch.empty_like(V), torch.empty_like(W)
    g = grid.desc()
    m = _operand(e, "grid metrics", grid.metrics(U.device), U, dtype=torch.float64, numel=3 * (grid.Ny + 2))
    _call(e, U.device, "fno_chanflow_rhs", C.byref(g), B, 0 if U.dtype == torch.float32 else 1, m, U, V, W, dp, dflt, Fu, Fv, Fw,
          STREAM)
    return Fu, Fv, Fw


class _ChanflowPdeLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, grid, U, Vgt, V, W):
        e = "chanflow_pde_loss"
        B = U.shape[0]
        U, Vgt, V, W = (_operand(e, n, t, U) for n, t in (("U", U), ("Vgt", Vgt), ("V", V), ("W", W)))
        g = grid.desc()
        nws = _lib.lib().fno_chanflow_pde_loss_workspace_bytes(C.byref(g), B)
        ws = _bytes(nws, U.device)
        loss = torch.empty(1, dtype=torch.float32, device=U.device)
        m = _operand(e, "grid metrics", grid.metrics(U.device), U, dtype=torch.float64, numel=3 * (grid.Ny + 2))
        _call("chanflow_pde_loss_forward", U.device, "fno_chanflow_pde_loss_forward", C.byref(g), B, m, U, Vgt, V, W, loss, ws,
              nws, STREAM)
        ctx.save_for_backward(U, Vgt, V, W, ws, m)
        ctx.meta = (grid, B, nws)
        return loss[0]

    @staticmethod
    def backward(ctx, gl):
        U, Vgt, V, W, ws, m = ctx.saved_tensors
        grid, B, nws = ctx.meta
        g = grid.desc()
        dV = torch.empty_like(V)
        glc = _operand("chanflow_pde_loss backward", "gl", gl.contiguous().to(torch.float32), V, numel=1).reshape(1)
        _call("chanflow_pde_loss_backward", V.device, "fno_chanflow_pde_loss_backward", C.byref(g), B, m, U, Vgt, V, W, glc, dV,
              ws, nws, STREAM)
        return None, None, None, dV, None


def chanflow_pde_loss(grid, U, Vgt, V, W):
    """sum_b ||Fu(U,Vgt,W) - Fu(U,V,W)|| + ||Fv ..|| + ||Fw ..||: NSControlEnvMatlab.pde_loss (libs/envs/control_env.py:627-633)
    summed over the batch as the training loop does (run_pde_observers.py:226-230).  fp32 fields on the GPU;
    differentiable w.r.t. V (the predicted wall-normal velocity); the pressure gradient cancels and is not an argument."""
    grid._check_fields(U, V, W, "chanflow_pde_loss")
    if tuple(Vgt.shape) != tuple(V.shape):
        raise RuntimeError(f"fnoengine chanflow_pde_loss: Vgt {tuple(Vgt.shape)} must match V {tuple(V.shape)}")
    _require_cuda(U, "U")
    return _ChanflowPdeLossFn.apply(grid, U, Vgt, V, W)


# ----------------------------------------------------------------------------
# channel-flow environment step, float64 (libs/envs/control_env.py:533-613, 196-229, 186-303)
# ----------------------------------------------------------------------------
CHANFLOW_DIAG = ("sum_div", "mean_abs_U", "mean_abs_V", "mean_abs_W", "norm_U", "norm_V", "norm_W", "shear_stress", "bulk_velocity",
                 "p2_mean", "dpdx_finite_difference", "shear_stress_signed")      # columns of chanflow_diagnostics


class ChannelPoisson:
    """The Poisson table of a ChannelGrid (fno_chanflow_poisson_pack): twiddles, bulk-velocity weights and the Thomas
    factors of every wavenumber pair's wall-normal system.  Built once on the host, one device copy per GPU."""

    def __init__(self, grid):
        import numpy as np
        self.grid = grid
        g = grid.desc()
        self.nbytes = int(_lib.lib().fno_chanflow_poisson_table_bytes(C.byref(g)))
        if self.nbytes == 0:
            raise RuntimeError("fnoengine ChannelPoisson: " + _lib.lib().fno_last_error().decode("utf-8", "replace"))
        self.packed = np.zeros(self.nbytes // 8, dtype=np.float64)
        dp = C.POINTER(C.c_double)
        _lib.check(_lib.lib().fno_chanflow_poisson_pack(C.byref(g), grid.y.ctypes.data_as(dp), grid.ym.ctypes.data_as(dp),
                                                        grid.yg.ctypes.data_as(dp), self.packed.ctypes.data_as(dp), self.nbytes),
                   "chanflow_poisson_pack")
        self._dev = {}

    def table(self, device):
        if device not in self._dev:
            self._dev[device] = torch.from_numpy(self.packed).to(device)
        return self._dev[device]

    def __getstate__(self):
        st = dict(self.__dict__)
        st["_dev"] = {}
        return st


def chanflow_step_workspace(grid, B, device):
    """an uninitialised workspace for `B` environments (every step entry point takes one; a graph holds on to its own)"""
    g = grid.desc()
    n = _lib.lib().fno_chanflow_step_workspace_bytes(C.byref(g), B)
    if n == 0:
        raise RuntimeError("fnoengine chanflow step: " + _lib.lib().fno_last_error().decode("utf-8", "replace"))
    return _bytes(n, device)


def _chanflow_step_operands(e, grid, poisson, U, V, W, ws, layout):
    """checked state, metrics, table and workspace of a step entry point.  dtype code 1 = float64; any other dtype and a table
    built for another grid reach the engine as they are, which refuses both before it launches anything"""
    grid._check_fields(U, V, W, e)
    dt = U.dtype
    code = {torch.float64: 1, torch.float32: 0}.get(dt, -1)
    U, V, W = (_operand(e, n, t, U, dtype=dt, layout=layout) for n, t in (("U", U), ("V", V), ("W", W)))
    m = _operand(e, "grid metrics", grid.metrics(U.device), U, dtype=torch.float64, numel=3 * (grid.Ny + 2))
    tab = _operand(e, "Poisson table", poisson.table(U.device), U, dtype=torch.float64)
    B = U.shape[0]
    if ws is None:
        ws = chanflow_step_workspace(grid, B, U.device)
    ws = _operand(e, "workspace", ws, U, dtype=torch.uint8, layout="dense")
    return B, code, U, V, W, m, tab, ws


def chanflow_project(grid, poisson, U, V, W, ws=None):
    """The fractional-step projection (compute_projection_step, control_env.py:582-613) of a batch of float64 states,
    IN PLACE: divergence, Poisson solve per wavenumber pair, gradient correction of the interior rows, then the U, W ghost
    rows by reflection (V's wall rows are left as they are).  Returns U, V, W."""
    e = "chanflow_project"
    B, code, U, V, W, m, tab, ws = _chanflow_step_operands(e, grid, poisson, U, V, W, ws, "dense")
    g = grid.desc()
    _call(e, U.device, "fno_chanflow_project", C.byref(g), B, code, m, tab, tab.numel() * 8, U, V, W, ws, ws.numel(), STREAM)
    return U, V, W


def chanflow_wall_pressure(grid, poisson, U, V, W, dPdx, full=False, ws=None, out=None):
    """p1, p2 (B, Nx, Nz) of get_boundary_pressures (control_env.py:423-427): the Poisson solve on the divergence of the
    right-hand side (:196-229), observed at the two walls; with full=True also P (B, Nx, Ny-1, Nz).  dPdx: float or (B,)
    float64 tensor.  `out` = (p1, p2[, P]) to write into existing tensors."""
    e = "chanflow_wall_pressure"
    B, code, U, V, W, m, tab, ws = _chanflow_step_operands(e, grid, poisson, U, V, W, ws, "copy")
    dp = _per_sample(e, "dPdx", dPdx, U)
    shp = (B, grid.Nx, grid.Nz)
    if out is None:
        out = [torch.empty(shp, dtype=torch.float64, device=U.device) for _ in range(2)]
        if full:
            out.append(torch.empty((B, grid.Nx, grid.Ny - 1, grid.Nz), dtype=torch.float64, device=U.device))
    p1, p2 = (_operand(e, n, t, U, dtype=torch.float64, shape=shp, layout="dense") for n, t in zip(("p1", "p2"), out))
    P = _operand(e, "P", out[2], U, dtype=torch.float64, shape=(B, grid.Nx, grid.Ny - 1, grid.Nz), layout="dense") if full else None
    g = grid.desc()
    _call(e, U.device, "fno_chanflow_wall_pressure", C.byref(g), B, code, m, tab, tab.numel() * 8, U, V, W, dp, p1, p2, P, ws,
          ws.numel(), STREAM)
    return (p1, p2, P) if full else (p1, p2)


def chanflow_rk3_step(grid, poisson, U, V, W, opV1, opV2, dPdx, meanU0, dt, ws=None):
    """One boundary-controlled RK3 step (time_advance_RK3_py, control_env.py:533-580) of a batch of float64 states, IN PLACE
    on U, V, W and on dPdx, a (B,) float64 tensor; opV1, opV2 (B, Nx, Nz) are the wall-normal velocities imposed at the two
    walls, meanU0 (B,) the bulk velocity the pressure gradient holds.  Nothing is read back: the step never synchronises."""
    e = "chanflow_rk3_step"
    B, code, U, V, W, m, tab, ws = _chanflow_step_operands(e, grid, poisson, U, V, W, ws, "dense")
    shp = (B, grid.Nx, grid.Nz)
    v1, v2 = (_operand(e, n, t, U, dtype=torch.float64, shape=shp) for n, t in (("opV1", opV1), ("opV2", opV2)))
    if not torch.is_tensor(dPdx):
        raise _refuse(e, "dPdx", "be a (B,) float64 tensor (it is updated in place)", type(dPdx).__name__)
    dp, mu = _per_sample(e, "dPdx", dPdx, U), _per_sample(e, "meanU0", meanU0, U)
    g = grid.desc()
    _call(e, U.device, "fno_chanflow_rk3_step", C.byref(g), B, code, m, tab, tab.numel() * 8, U, V, W, v1, v2, dp, mu, float(dt), ws,
          ws.numel(), STREAM)
    return U, V, W, dp


def chanflow_diagnostics(grid, poisson, U, V, W, p2=None, out=None):
    """(B, 12) float64, columns CHANFLOW_DIAG: the scalars of the environment's `info` (control_env.py:186-303) in one launch;
    p2 (B, Nx, Nz) feeds the two pressure columns (0 without it)."""
    e = "chanflow_diagnostics"
    grid._check_fields(U, V, W, e)
    dt = U.dtype
    U, V, W = (_operand(e, n, t, U, dtype=dt) for n, t in (("U", U), ("V", V), ("W", W)))
    B = U.shape[0]
    m = _operand(e, "grid metrics", grid.metrics(U.device), U, dtype=torch.float64, numel=3 * (grid.Ny + 2))
    tab = _operand(e, "Poisson table", poisson.table(U.device), U, dtype=torch.float64)
    p2 = _operand(e, "p2", p2, U, dtype=torch.float64, shape=(B, grid.Nx, grid.Nz), optional=True)
    if out is None:
        out = torch.empty((B, len(CHANFLOW_DIAG)), dtype=torch.float64, device=U.device)
    out = _operand(e, "out", out, U, dtype=torch.float64, shape=(B, len(CHANFLOW_DIAG)), layout="dense")
    g = grid.desc()
    _call(e, U.device, "fno_chanflow_diagnostics", C.byref(g), B, {torch.float64: 1, torch.float32: 0}.get(dt, -1), m, tab,
          tab.numel() * 8, U, V, W, p2, out, STREAM)
    return out


class GraphedChannelStep:
    """chanflow_rk3_step + chanflow_wall_pressure of a fixed batch replayed as ONE graph.  The state, the controls, dPdx and
    the observations live in tensors the graph owns: write `opV1` / `opV2` (copy_), call step(), read `p1` / `p2`."""

    def __init__(self, grid, poisson, U, V, W, dPdx, meanU0, dt):
        self.grid, self.poisson, self.dt = grid, poisson, float(dt)
        self.U, self.V, self.W = (t.detach().clone().contiguous() for t in (U, V, W))
        B, dev = self.U.shape[0], self.U.device
        self.dPdx, self.meanU0 = _per_sample("GraphedChannelStep", "dPdx", dPdx, self.U).clone(), _per_sample("GraphedChannelStep", "meanU0", meanU0, self.U).clone()
        self.opV1 = torch.zeros((B, grid.Nx, grid.Nz), dtype=torch.float64, device=dev)
        self.opV2 = torch.zeros_like(self.opV1)
        self.p1, self.p2 = torch.zeros_like(self.opV1), torch.zeros_like(self.opV1)
        self.ws = chanflow_step_workspace(grid, B, dev)
        saved = [t.clone() for t in (self.U, self.V, self.W, self.dPdx)]
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):                      # one eager run loads the code objects before the capture
            self._body()
        torch.cuda.current_stream(dev).wait_stream(side)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self._body()
        for t, s in zip((self.U, self.V, self.W, self.dPdx), saved):
            t.copy_(s)

    def _body(self):
        chanflow_rk3_step(self.grid, self.poisson, self.U, self.V, self.W, self.opV1, self.opV2, self.dPdx, self.meanU0, self.dt,
                          ws=self.ws)
        chanflow_wall_pressure(self.grid, self.poisson, self.U, self.V, self.W, self.dPdx, ws=self.ws, out=(self.p1, self.p2))

    def step(self):
        self.graph.replay()
        return self.p1, self.p2


# ----------------------------------------------------------------------------
# closed-loop control (run_control.py): two-level diagnostics
# ----------------------------------------------------------------------------
CONTROL_LOG = CHANFLOW_DIAG + ("dPdx",)      # columns of chanflow_diagnostics2: one row of a (T, B, 13) control log


def chanflow_diagnostics2_workspace(grid, B, device):
    """the partial-sum workspace of chanflow_diagnostics2 for `B` environments on this grid (its size is checked exactly)"""
    g = grid.desc()
    n = _lib.lib().fno_chanflow_diagnostics2_workspace_bytes(C.byref(g), B)
    if n == 0:
        raise RuntimeError("fnoengine chanflow_diagnostics2: " + _lib.lib().fno_last_error().decode("utf-8", "replace"))
    return torch.empty(n, dtype=torch.uint8, device=device)


def chanflow_diagnostics2(grid, poisson, U, V, W, p2, dPdx, out=None, ws=None):
    """(B, 13) float64, columns CONTROL_LOG: chanflow_diagnostics and dPdx as a two-level reduction (a workgroup per wall-normal
    row and sample, then one per sample in a fixed order), written straight into `out`: a (B, 13) tensor or one row log[r] of a
    (T, B, 13) device log.  dPdx: the (B,) float64 device tensor of the step.  `ws`: chanflow_diagnostics2_workspace of this
    grid and batch."""
    e = "chanflow_diagnostics2"
    grid._check_fields(U, V, W, e)
    dt = U.dtype
    U, V, W = (_operand(e, n, t, U, dtype=dt) for n, t in (("U", U), ("V", V), ("W", W)))
    B, ncol = U.shape[0], len(CONTROL_LOG)
    m = _operand(e, "grid metrics", grid.metrics(U.device), U, dtype=torch.float64, numel=3 * (grid.Ny + 2))
    tab = _operand(e, "Poisson table", poisson.table(U.device), U, dtype=torch.float64)
    p2 = _operand(e, "p2", p2, U, dtype=torch.float64, shape=(B, grid.Nx, grid.Nz), optional=True)
    if not torch.is_tensor(dPdx):
        raise _refuse(e, "dPdx", "be a (B,) float64 tensor", type(dPdx).__name__)
    dp = _per_sample(e, "dPdx", dPdx, U)
    if out is None:
        out = torch.empty((B, ncol), dtype=torch.float64, device=U.device)
    out = _operand(e, "out", out, U, dtype=torch.float64, shape=(B, ncol), layout="keep")
    stride = out.stride(0) if B > 1 else ncol
    if out.stride(1) != 1 or stride < ncol:
        raise _refuse(e, "out", "have unit-stride rows at least 13 apart", f"strides {out.stride()}")
    g = grid.desc()
    need = _lib.lib().fno_chanflow_diagnostics2_workspace_bytes(C.byref(g), B)
    if ws is None:
        ws = chanflow_diagnostics2_workspace(grid, B, U.device)
    ws = _operand(e, "workspace", ws, U, dtype=torch.uint8, layout="dense")
    if ws.numel() != need:
        raise _refuse(e, "workspace", f"be the {need} bytes of this grid and a batch of {B}", f"{ws.numel()} bytes")
    _call(e, U.device, "fno_chanflow_diagnostics2", C.byref(g), B, {torch.float64: 1, torch.float32: 0}.get(dt, -1), m, tab,
          tab.numel() * 8, U, V, W, p2, dp, out, stride, ws, ws.numel(), STREAM)
    return out
