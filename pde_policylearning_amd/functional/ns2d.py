"""The 2-D channel solver of NSControlEnv2D (fp64): grid, steady solve, fixed-mass-flow solve, diagnostics.
"""
import ctypes as C
import typing

import torch

from .. import _lib
from ._core import _call, _gpu_anchor, _operand, _per_sample, _refuse, STREAM


# ----------------------------------------------------------------------------
# NSControlEnv2D: the 2-D periodic channel (libs/envs/ns_control_2d.py), float64, one workgroup per environment
# ----------------------------------------------------------------------------
NS2D_SOLVE_OUT = ("bulk_v", "steps", "status")
NS2D_STATUS = ("converged", "max_step", "cap")
NS2D_FIXED_OUT = ("result_f", "flow", "error", "bisections", "steps", "status")
NS2D_FIXED_STATUS = ("ok", "overflow", "cap")
NS2D_DIAG = ("drag_reduction/1_shear_stress", "drag_reduction/2_1_mass_flow", "drag_reduction/2_2_v_velocity",
             "drag_reduction/3_1_pressure_mean", "drag_reduction/3_2_dPdx_required", "drag_reduction/4_1_-|divergence|",
             "drag_reduction/4_2_speed_norm")


class Ns2dGrid(typing.NamedTuple):
    """(ny, nx) points, periodic in x with all nx columns distinct, walls at rows 0 and ny-1; nit Jacobi sweeps per step"""
    nx: int
    ny: int
    nit: int
    dx: float
    dy: float
    dt: float
    rho: float

    def desc(self):
        return _lib.FnoNs2dGrid(int(self.nx), int(self.ny), int(self.nit), float(self.dx), float(self.dy), float(self.dt),
                                float(self.rho))


def _ns2d_operands(e, grid, p, u, v, nu, bc_lo, bc_hi, layout):
    """checked state, viscosity and wall rows of an ns2d entry point; the grid's extents reach the engine as they are, which
    refuses what it does not support before it launches anything"""
    _gpu_anchor(e, "p", p)
    if p.dim() != 3 or tuple(p.shape[1:]) != (grid.ny, grid.nx):
        raise _refuse(e, "p", f"be (B, {grid.ny}, {grid.nx}), the grid's (B, ny, nx)", tuple(p.shape))
    B = p.shape[0]
    p, u, v = (_operand(e, n, t, p, dtype=torch.float64, shape=p.shape, layout=layout) for n, t in (("p", p), ("u", u), ("v", v)))
    nu = _per_sample(e, "nu", nu, p)
    lo, hi = (_operand(e, n, t, p, dtype=torch.float64, shape=(B, grid.nx), optional=True) for n, t in (("bc_lo", bc_lo), ("bc_hi", bc_hi)))
    return B, p, u, v, nu, lo, hi


def ns2d_solve(grid, p, u, v, F, nu, bc_lo=None, bc_hi=None, max_step=-1, u_diff_thre=1e-2, step_cap=5000, update_state=True,
               un=None, vn=None, out=None):
    """NSControlEnv2D.solve (ns_control_2d.py:359-491) of a batch of float64 states (B, ny, nx) in one launch: F, nu floats or
    (B,) tensors, bc_lo / bc_hi (B, nx) wall-normal velocities at rows 0 / ny-1 (None: zero).  Steps while
    udiff > u_diff_thre; max_step > 1 caps (so 1 and -1 run to convergence, as the reference), more than step_cap steps end
    the launch.  update_state: p, u, v are advanced IN PLACE (and un, vn written when given) unless the cap was hit.
    Returns (B, 3) float64, columns NS2D_SOLVE_OUT; status indexes NS2D_STATUS.  Nothing is read back here."""
    e = "ns2d_solve"
    B, p, u, v, nu, lo, hi = _ns2d_operands(e, grid, p, u, v, nu, bc_lo, bc_hi, "dense" if update_state else "copy")
    F = _per_sample(e, "F", F, p)
    un, vn = (_operand(e, n, t, p, dtype=torch.float64, shape=p.shape, optional=True, layout="dense") for n, t in (("un", un), ("vn", vn)))
    if out is None:
        out = torch.empty((B, len(NS2D_SOLVE_OUT)), dtype=torch.float64, device=p.device)
    out = _operand(e, "out", out, p, dtype=torch.float64, shape=(B, len(NS2D_SOLVE_OUT)), layout="dense")
    g = grid.desc()
    _call(e, p.device, "fno_ns2d_solve", C.byref(g), B, p, u, v, un, vn, F, nu, lo, hi, int(max_step), float(u_diff_thre),
          int(step_cap), int(bool(update_state)), out, STREAM)
    return out


def ns2d_fixed_mass(grid, p, u, v, F, nu, target, min_f, max_f, bc_lo=None, bc_hi=None, u_diff_thre=1e-2, step_cap=5000,
                    max_bisect=500, error_threshold=1e-4, out=None):
    """NSControlEnv2D.solve_fixed_mass (:493-536) in one launch: converged solves at min_f and max_f from the given state, then
    bisection on the force towards the bulk velocity `target`; F is what a target outside the bracket returns.  Every
    per-environment scalar is a float or a (B,) tensor.  The state is read only.  Returns (B, 6) float64, columns
    NS2D_FIXED_OUT; status indexes NS2D_FIXED_STATUS."""
    e = "ns2d_fixed_mass"
    B, p, u, v, nu, lo, hi = _ns2d_operands(e, grid, p, u, v, nu, bc_lo, bc_hi, "copy")
    F, target, min_f, max_f = (_per_sample(e, n, t, p) for n, t in (("F", F), ("target", target), ("min_f", min_f), ("max_f", max_f)))
    if out is None:
        out = torch.empty((B, len(NS2D_FIXED_OUT)), dtype=torch.float64, device=p.device)
    out = _operand(e, "out", out, p, dtype=torch.float64, shape=(B, len(NS2D_FIXED_OUT)), layout="dense")
    g = grid.desc()
    _call(e, p.device, "fno_ns2d_fixed_mass", C.byref(g), B, p, u, v, F, nu, target, min_f, max_f, lo, hi, float(u_diff_thre),
          int(step_cap), int(max_bisect), float(error_threshold), out, STREAM)
    return out


def ns2d_diagnostics(grid, p, u, v, nu, dpdx=None, out=None, ptop=None):
    """The seven drag_reduction scalars of NSControlEnv2D.step (:562-581) as (B, 7) float64, columns NS2D_DIAG, and the top-wall
    pressure row p[:, -1, :] as (B, nx); dpdx: (B,) tensor or float for drag_reduction/3_2_dPdx_required (None: -1)."""
    e = "ns2d_diagnostics"
    B, p, u, v, nu, _, _ = _ns2d_operands(e, grid, p, u, v, nu, None, None, "copy")
    dpdx = None if dpdx is None else _per_sample(e, "dpdx", dpdx, p)
    if out is None:
        out = torch.empty((B, len(NS2D_DIAG)), dtype=torch.float64, device=p.device)
    out = _operand(e, "out", out, p, dtype=torch.float64, shape=(B, len(NS2D_DIAG)), layout="dense")
    if ptop is None:
        ptop = torch.empty((B, grid.nx), dtype=torch.float64, device=p.device)
    ptop = _operand(e, "ptop", ptop, p, dtype=torch.float64, shape=(B, grid.nx), layout="dense")
    g = grid.desc()
    _call(e, p.device, "fno_ns2d_diagnostics", C.byref(g), B, p, u, v, nu, dpdx, out, ptop, STREAM)
    return out, ptop
