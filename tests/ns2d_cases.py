"""Helpers of the NSControlEnv2D tests (a helper module, not a conftest): a numpy restatement of the reference's 2-D channel
solver, the case table and the tolerance rule.

The restatement follows libs/envs/ns_control_2d.py expression by expression (the cited lines), with the three column blocks of
every update (interior, x = 2, x = 0) written once through np.roll: the same operations in the same order on every point, so in
float64 it gives the reference's bits wherever numpy's vector arithmetic does.  It is generic in the dtype: run in
np.longdouble it is the second evaluation the floors are taken from.

The rule is the float64 floor rule of tests/judging.py: bound = min(16 * max(floor, eps), 1e-9), the floor of a compared field
being the max-norm distance between the float64 and the long-double restatement divided by max|field|.  Nothing is tuned to
what the kernels give.  Every distance, floor and bound goes to profiles/r15_ns2d_errors.txt before anything is asserted."""
import functools
import os

import numpy as np

from tests.judging import EPS64 as EPS, SectionLog, bound, judge_floor  # noqa: F401  (re-exported to the tests)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOG = SectionLog(os.path.join(ROOT, "profiles", "r15_ns2d_errors.txt"))
log_block = LOG.replace
judge = functools.partial(judge_floor, LOG)
INFO_KEYS = ("drag_reduction/1_shear_stress", "drag_reduction/2_1_mass_flow", "drag_reduction/2_2_v_velocity",
             "drag_reduction/3_1_pressure_mean", "drag_reduction/3_2_dPdx_required", "drag_reduction/4_1_-|divergence|",
             "drag_reduction/4_2_speed_norm")


class Grid:
    """ns_control_2d.py:78-92 with nx, ny free: dx = 2 / (nx - 1), dy = 2 / (ny - 1), dt = 0.01, rho = 1, nit = 50"""

    def __init__(self, ny, nx, nit=50, dt=0.01, rho=1.0):
        self.ny, self.nx, self.nit, self.dt, self.rho = ny, nx, nit, dt, rho
        self.dx, self.dy = 2 / (nx - 1), 2 / (ny - 1)

    def engine(self):
        from pde_policylearning_amd import functional as F
        return F.Ns2dGrid(self.nx, self.ny, self.nit, self.dx, self.dy, self.dt, self.rho)


def _lr(a):
    """right and left neighbours along the periodic x axis: column 0 and column nx-1 are neighbours (:22-36)"""
    return np.roll(a, -1, axis=1), np.roll(a, 1, axis=1)


def build_up_b(rho, dt, dx, dy, u, v):
    """:13-38"""
    b = np.zeros_like(u)
    ur, ul = _lr(u[1:-1])
    vr, vl = _lr(v[1:-1])
    b[1:-1] = (rho * (1 / dt * ((ur - ul) / (2 * dx) + (v[2:] - v[:-2]) / (2 * dy)) -
                      ((ur - ul) / (2 * dx))**2 -
                      2 * ((u[2:] - u[:-2]) / (2 * dy) * (vr - vl) / (2 * dx)) -
                      ((v[2:] - v[:-2]) / (2 * dy))**2))
    return b


def pressure_poisson_periodic(p, dx, dy, b, nit):
    """:41-67"""
    for _ in range(nit):
        pn = p.copy()
        pr, pl = _lr(pn[1:-1])
        p[1:-1] = (((pr + pl) * dy**2 + (pn[2:] + pn[:-2]) * dx**2) / (2 * (dx**2 + dy**2)) -
                   dx**2 * dy**2 / (2 * (dx**2 + dy**2)) * b[1:-1])
        p[-1, :] = p[-2, :]
        p[0, :] = p[1, :]
    return p


def solve(g, state, bc, max_step, nu, F, u_diff_thre=1e-2, step_cap=5000, dtype=np.float64, history=None):
    """NSControlEnv2D.solve (:359-491) from state = (p, u, v).  Returns a dict: p, u, v, un, vn, bulk_v, steps and status
    ("converged" / "max_step" / "cap": where the reference raises "Not converged solving!" this returns after the same
    step_cap + 1 steps).  history: a list that receives every udiff."""
    T = np.dtype(dtype).type
    p, u, v = (np.array(a, dtype=dtype) for a in state)
    dx, dy, dt, rho, nu, F = T(g.dx), T(g.dy), T(g.dt), T(g.rho), T(nu), T(F)
    lo, hi = (0, 0) if bc is None else bc
    lo, hi = np.asarray(lo, dtype=dtype), np.asarray(hi, dtype=dtype)
    un, vn = u.copy(), v.copy()
    udiff, steps, status = 1.0, 0, "converged"
    while udiff > u_diff_thre:
        u[0, :] = 0
        u[-1, :] = 0
        v[0, :] = lo
        v[-1, :] = hi
        un = u.copy()
        vn = v.copy()
        b = build_up_b(rho, dt, dx, dy, u, v)
        p = pressure_poisson_periodic(p, dx, dy, b, g.nit)
        c, cd, cu = un[1:-1], un[:-2], un[2:]
        w, wd, wu = vn[1:-1], vn[:-2], vn[2:]
        cr, cl = _lr(c)
        wr, wl = _lr(w)
        pr, pl = _lr(p[1:-1])
        u[1:-1] = (c - c * dt / dx * (c - cl) - w * dt / dy * (c - cd) - dt / (2 * rho * dx) * (pr - pl) +
                   nu * (dt / dx**2 * (cr - 2 * c + cl) + dt / dy**2 * (cu - 2 * c + cd)) + F * dt)
        v[1:-1] = (w - c * dt / dx * (w - wl) - w * dt / dy * (w - wd) - dt / (2 * rho * dy) * (p[2:] - p[:-2]) +
                   nu * (dt / dx**2 * (wr - 2 * w + wl) + dt / dy**2 * (wu - 2 * w + wd)))
        udiff = (np.sum(u) - np.sum(un)) / np.sum(u)
        if history is not None:
            history.append(float(udiff))
        steps += 1
        if steps > step_cap:
            status = "cap"
            break
        if max_step > 1 and steps >= max_step:
            status = "max_step"
            break
    return {"p": p, "u": u, "v": v, "un": un, "vn": vn, "bulk_v": np.mean(abs(u)), "steps": steps, "status": status}


def solve_fixed_mass(g, state, bc, target, min_f, max_f, nu, F, max_step=500, error_threshold=1e-4, dtype=np.float64, **kw):
    """solve_fixed_mass (:493-536).  Returns a dict: result_f, flow, error, bisections, steps (of all solves), status
    ("ok" / "overflow") and trace = [(mid_f, flow, error)] per bisection."""
    T = np.dtype(dtype).type
    run = lambda f: solve(g, state, bc, -1, nu, f, dtype=dtype, **kw)
    lo, hi = run(min_f), run(max_f)
    total = lo["steps"] + hi["steps"]
    if target < lo["bulk_v"] or target > hi["bulk_v"]:
        return {"result_f": F, "flow": target, "error": 0, "bisections": 0, "steps": total, "status": "overflow", "trace": []}
    min_f, max_f = T(min_f), T(max_f)
    step, error, result_f, flow, trace = 0, float("inf"), None, 0, []
    while step < max_step and error > error_threshold:
        mid_f = (min_f + max_f) / 2
        r = run(mid_f)
        total += r["steps"]
        flow = r["bulk_v"]
        error = abs(flow - target)
        if flow < target:
            min_f = mid_f
        else:
            max_f = mid_f
        result_f = mid_f
        step += 1
        trace.append((float(mid_f), float(flow), float(error)))
    return {"result_f": result_f, "flow": flow, "error": error, "bisections": step, "steps": total, "status": "ok", "trace": trace}


def seeded_start(ny=41, nx=41, seed=0):
    """the reference's start (:99-101) after np.random.seed(seed): p, u, v"""
    np.random.seed(seed)
    u = np.ones((ny, nx)) * 1.0
    v = np.ones((ny, nx)) * 0.15 + np.random.rand(ny, nx) * 0.1
    return v.copy(), u, v


class Restated:
    """The environment (:70-107, :546-586) on the restatement, one environment."""

    def __init__(self, Re, fix_flow, g=None, init_v=None, dtype=np.float64):
        self.g, self.fix_flow, self.dtype = g or Grid(41, 41), fix_flow, dtype
        if init_v is None:
            init_v = np.ones((self.g.ny, self.g.nx)) * 0.15 + np.random.rand(self.g.ny, self.g.nx) * 0.1
        self.u = np.ones((self.g.ny, self.g.nx), dtype=dtype)
        self.v = np.array(init_v, dtype=dtype)
        self.p = self.v.copy()
        self.F = 4.0
        self.nu = self.u.max() / Re
        self.init_steps = self._solve(None, -1)["steps"]
        self.init_bulk_v = None
        self.info_init = None
        self.fixed = []

    def _solve(self, bc, max_step):
        r = solve(self.g, (self.p, self.u, self.v), bc, max_step, self.nu, self.F, dtype=self.dtype)
        self.p, self.u, self.v, self.un, self.vn = r["p"], r["u"], r["v"], r["un"], r["vn"]
        return r

    def gt_control(self):
        return [0, -self.v[-10, :]]

    def step(self, bc):
        self._solve(bc, 3)
        if self.init_bulk_v is None:
            self.init_bulk_v = np.mean(abs(self.u))
            self.info_init = None
        if self.fix_flow:
            fm = solve_fixed_mass(self.g, (self.p, self.u, self.v), bc, self.init_bulk_v, 0, 3 * self.F, self.nu, self.F, dtype=self.dtype)
            self.fixed.append(fm)
            self.F = dpdx = fm["result_f"]
        else:
            dpdx = -1
        u, v, p = self.u, self.v, self.p
        ptop = p[-1, :]
        div = (u[10, 10] - u[9, 10]) / self.g.dx + (v[10, 10] - v[10, 9]) / self.g.dy            # cal_div (:169-172)
        reward = max(-abs(div), -100)                                                           # reward_div (:225-229)
        shear = abs(np.mean(-u[-1, :] * v[-1, :] + self.nu * ((u[-2, :] - u[-3, :]) / self.g.dy)))   # (:205-223)
        info = dict(zip(INFO_KEYS, (shear, abs(u).mean(), abs(v).mean(), ptop.mean(), dpdx, reward,
                                    np.linalg.norm(v) + np.linalg.norm(u))))
        if self.info_init is None:                                                              # cal_relative_info (:249-258)
            self.info_init = dict(info)
        else:
            info.update({k.replace("drag_reduction", "drag_reduction_relative"): info[k] / (self.info_init[k] + 1e-9) for k in INFO_KEYS})
        return ptop, reward, False, info


def info_scales(env):
    """what one rounding of each cancelling info entry is relative to (entries not listed: their own magnitude)"""
    u, v, g = np.asarray(env.u, dtype=np.float64), np.asarray(env.v, dtype=np.float64), env.g
    return {"drag_reduction/4_1_-|divergence|": (abs(u[10, 10]) + abs(u[9, 10])) / g.dx + (abs(v[10, 10]) + abs(v[10, 9])) / g.dy,
            "drag_reduction/1_shear_stress": float(np.mean(abs(u[-1] * v[-1]) + abs(env.nu) * (abs(u[-2]) + abs(u[-3])) / g.dy)),
            "drag_reduction/3_1_pressure_mean": float(np.abs(np.asarray(env.p, dtype=np.float64)[-1]).mean())}


def rel(a, b):
    """max-norm distance relative to max|b|"""
    a, b = np.asarray(a, dtype=np.longdouble), np.asarray(b, dtype=np.longdouble)
    den = np.max(np.abs(b))
    return float(np.max(np.abs(a - b)) / (den if den > 0 else 1.0))


# ---------------------------------------------------------------------------------------------------------------------------
# the case table
# ---------------------------------------------------------------------------------------------------------------------------
CAPPED_GRIDS = [(6, 7), (9, 12), (41, 41), (33, 64)]          # (ny, nx): wrap-around columns next to wall rows; a row length
CAPPED_F = (0.0, 4.0, 12.0)                                   # that is no multiple of the wave; more than one point per thread
CAPPED_NU = (1 / 1000, 1 / 3000, 1 / 5000)


def capped_case(ny, nx):
    """B = 3 states with per-environment walls: arrays on both walls / scalar 0 below with an array above / none"""
    rng = np.random.default_rng(1000 * ny + nx)
    states = []
    for _ in range(3):
        v = 0.15 + 0.1 * rng.random((ny, nx))
        states.append((v.copy(), np.ones((ny, nx)), v))
    a0, a1, a2 = (0.05 * (rng.random(nx) - 0.5) for _ in range(3))
    return states, [(a0, a1), (0, a2), None]


def bc_rows(bcs, nx):
    """per-environment bc -> the (B, nx) rows of the engine"""
    lo = np.stack([np.zeros(nx) if b is None else np.broadcast_to(np.asarray(b[0], dtype=np.float64), (nx,)) for b in bcs])
    hi = np.stack([np.zeros(nx) if b is None else np.broadcast_to(np.asarray(b[1], dtype=np.float64), (nx,)) for b in bcs])
    return lo, hi


def small_start(ny=9, nx=12, seed=5):
    rng = np.random.default_rng(seed)
    v = 0.15 + 0.1 * rng.random((ny, nx))
    return v.copy(), np.ones((ny, nx)), v
