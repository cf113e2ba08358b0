"""Float64 CPU restatement of the channel-flow environment step (a helper module for the tests, not a conftest).

Written from the equations of the fractional-step scheme on the staggered grid:
  divergence      d[i,j,k] = (U[i+1,j+1,k]-U[i,j+1,k])/dx + (V[i,j+1,k]-V[i,j,k])/(y[j+1]-y[j]) + (W[i,j+1,k+1]-W[i,j+1,k])/dz
  Poisson         fft over z and x; per wavenumber pair the (Ny-1)x(Ny-1) system (DD + (kxx[kx]+kzz[kz]) I) p_hat = d_hat with
                  modified wavenumbers 2 (cos(2 pi k/N) - 1)/h^2, DD the wall-normal second difference with Neumann ends, and
                  the (0,0) system's first diagonal entry x 1.5
  correction      U -= dp/dx, V[1:-1] -= dp/dy (centre spacing), W -= dp/dz on the interior rows
  wall condition  U, W ghost rows by reflection, V wall rows = the control
  RK3             X0 + dt 8/15 F1;  X0 + dt (1/4 F1 + 5/12 F2);  X0 + dt (1/4 F1 + 3/4 F3), each projected between wall conditions
  bulk velocity   trapezoid over [0, ym, 2] of the xz-mean profile, / 2;  U[1:-1] += dPdx_new/2;  dPdx = (dPdx + dPdx_new/dt)/2
The Poisson systems are solved by DENSE numpy.linalg.solve per wavenumber (`solver="dense"`), so that the restatement shares
neither algorithm nor table with the kernels; `solver="thomas"` is a float64 Thomas recurrence on the same matrices, used
only to measure the floor the GPU tolerances are derived from.  The right-hand side comes from oracle.chanflow_oracle.
Fields are numpy float64: U, W (Nx, Ny+1, Nz), V (Nx, Ny, Nz)."""
import numpy as np
import torch

from oracle import chanflow_oracle as Co

NU = 3.076923076923077e-04
DPDX0 = 0.57231059E-01 ** 2
INFO_KEYS = ["drag_reduction/1_shear_stress", "drag_reduction/2_1_mass_flow", "drag_reduction/2_2_v_velocity",
             "drag_reduction/2_3_w_velocity", "drag_reduction/3_1_pressure_mean",
             "drag_reduction/3_2_dPdx_finite_difference", "drag_reduction/3_3_dPdx_reverse_cal",
             "drag_reduction/4_1_-|divergence|", "drag_reduction/4_4_speed_norm"]


class Grid:
    def __init__(self, Nx, Ny, Nz, Lx=2 * np.pi, Lz=2 * np.pi, nu=NU):
        self.Nx, self.Ny, self.Nz = Nx, Ny, Nz
        self.dx, self.dz, self.nu = Lx / Nx, Lz / Nz, nu
        self.y, self.ym, self.yg = Co.tanh_grid(Ny)
        self.kxx = self._kmod(Nx, self.dx)
        self.kzz = self._kmod(Nz, self.dz)
        n = Ny - 1
        hy, hg = np.diff(self.y), np.diff(self.yg)             # hy[j] = y[j+1]-y[j];  hg[j] = yg[j+1]-yg[j]
        DD = np.zeros((n, n))
        DD[np.arange(n), np.arange(n)] = -(1 / hg[1:] + 1 / hg[:-1]) / hy
        DD[np.arange(1, n), np.arange(n - 1)] = 1 / hy[1:] / hg[1:-1]
        DD[np.arange(n - 1), np.arange(1, n)] = 1 / hy[:-1] / hg[1:-1]
        DD[0, 0] += 1 / hy[0] / hg[0]
        DD[-1, -1] += 1 / hy[-1] / hg[-1]
        self.DD = DD

    @staticmethod
    def _kmod(N, h):
        k = np.arange(N)
        k = np.where(k <= N // 2, k, k - N)
        return 2 * (np.cos(2 * np.pi * k / N) - 1) / h ** 2

    def matrix(self, i, k):
        D = self.DD + np.eye(self.Ny - 1) * (self.kxx[i] + self.kzz[k])
        if i == 0 and k == 0:
            D[0, 0] *= 1.5
        return D


def divergence(g, U, V, W):
    hy = np.diff(g.y)[None, :, None]
    return (np.roll(U, -1, 0) - U)[:, 1:-1] / g.dx + (V[:, 1:] - V[:, :-1]) / hy + (np.roll(W, -1, 2) - W)[:, 1:-1] / g.dz


def _thomas(D, r):
    n = D.shape[0]
    a, b, c = np.diag(D, -1), np.diag(D), np.diag(D, 1)
    cp, dp = np.zeros(n), np.zeros(n, dtype=r.dtype)
    cp[0], dp[0] = c[0] / b[0], r[0] / b[0]
    for j in range(1, n):
        m = b[j] - a[j - 1] * cp[j - 1]
        if j < n - 1:
            cp[j] = c[j] / m
        dp[j] = (r[j] - a[j - 1] * dp[j - 1]) / m
    x = np.zeros(n, dtype=r.dtype)
    x[-1] = dp[-1]
    for j in range(n - 2, -1, -1):
        x[j] = dp[j] - cp[j] * x[j + 1]
    return x


def poisson(g, d, solver="dense"):
    """(p, p_hat) with p_hat (Nx, Ny-1, Nz) the solved spectrum of the divergence field d."""
    h = np.fft.fft(np.fft.fft(d, axis=2), axis=0)
    for i in range(g.Nx):
        for k in range(g.Nz):
            D = g.matrix(i, k)
            h[i, :, k] = np.linalg.solve(D.astype(complex), h[i, :, k]) if solver == "dense" else _thomas(D, h[i, :, k])
    return np.real(np.fft.ifft(np.fft.ifft(h, axis=0), axis=2)), h


def wall_condition(U, V, W, v1=None, v2=None):
    U, V, W = U.copy(), V.copy(), W.copy()
    U[:, 0], U[:, -1] = -U[:, 1], -U[:, -2]
    W[:, 0], W[:, -1] = -W[:, 1], -W[:, -2]
    if v1 is not None:
        V[:, 0], V[:, -1] = v1, v2
    return U, V, W


def project_raw(g, U, V, W, solver="dense"):
    """the fractional step alone: (U, V, W, p_hat) without the wall condition"""
    p, ph = poisson(g, divergence(g, U, V, W), solver)
    U, V, W = U.copy(), V.copy(), W.copy()
    U[:, 1:-1] -= (p - np.roll(p, 1, 0)) / g.dx
    V[:, 1:-1] -= (p[:, 1:] - p[:, :-1]) / np.diff(g.ym)[None, :, None]
    W[:, 1:-1] -= (p - np.roll(p, 1, 2)) / g.dz
    return U, V, W, ph


def project(g, U, V, W, solver="dense"):
    """what the engine's chanflow_project computes: the fractional step, then the U, W ghost rows by reflection"""
    U, V, W, ph = project_raw(g, U, V, W, solver)
    return wall_condition(U, V, W) + (ph,)


def rhs(g, U, V, W, dPdx):
    t = torch.from_numpy
    return tuple(f.numpy() for f in Co.compute_rhs(t(U), t(V), t(W), float(dPdx), g.dx, g.dz, g.y, g.ym, g.yg, g.nu))


def bulk_velocity(g, U):
    prof = U[:, 1:-1].mean(axis=2).mean(axis=0)
    f, x = np.concatenate(([0.0], prof, [0.0])), np.concatenate(([0.0], g.ym, [2.0]))
    return float(np.sum(0.5 * (f[1:] + f[:-1]) * np.diff(x)) / 2)


def rk3_step(g, U0, V0, W0, v1, v2, dPdx, meanU0, dt, solver="dense"):
    def stage(ca, F1, cb=0.0, Fs=None):
        X = [x0 + dt * (ca * f1 + (cb * fs if Fs is not None else 0.0)) for x0, f1, fs in zip((U0, V0, W0), F1, Fs or F1)]
        X = wall_condition(*X, v1, v2)
        X = project_raw(g, *X, solver)[:3]
        return wall_condition(*X, v1, v2)
    F1 = rhs(g, U0, V0, W0, dPdx)
    X = stage(8 / 15, F1)
    X = stage(1 / 4, F1, 5 / 12, rhs(g, *X, dPdx))
    U, V, W = stage(1 / 4, F1, 3 / 4, rhs(g, *X, dPdx))
    new = 2 * (meanU0 - bulk_velocity(g, U))
    U[:, 1:-1] += new / 2
    return U, V, W, 0.5 * (dPdx + new / dt)


def pressure(g, U, V, W, dPdx, solver="dense"):
    """(p1, p2, P): the Poisson solve on the divergence of the right-hand side and the two wall observations"""
    P, _ = poisson(g, divergence(g, *rhs(g, U, V, W, dPdx)), solver)
    return -0.5 * (P[:, 0] + P[:, 1]), -0.5 * (P[:, -1] + P[:, -2]), P


def gt_control(V, detect_plane):
    return -V[:, detect_plane, :].copy(), -V[:, -detect_plane, :].copy()


def step_info(g, U, V, W, p2, dPdx):
    """the `info` of one environment step, keyed like the reference's"""
    dudy = (U[:, -2] - U[:, -3]) / (g.y[-1] - g.y[-2])
    shear = abs(np.mean(-U[:, -1] * V[:, -1] + g.nu * dudy))
    fd = abs(np.mean([np.abs((p2[i + 1] - p2[i]) / g.dx).mean() for i in range(g.Nx - 1)]))
    div = -abs(np.sum(divergence(g, U, V, W)))
    vals = [shear, bulk_velocity(g, U), np.abs(V).mean(), np.abs(W).mean(), p2.mean(), fd, dPdx, max(div, -100.0),
            np.linalg.norm(V) + np.linalg.norm(U) + np.linalg.norm(W)]
    return dict(zip(INFO_KEYS, (float(v) for v in vals)))


def analytic_state(g, seed, noise=0.05, B=None):
    """a parabolic streamwise profile plus seeded noise, wall condition applied (V walls included: random wall planes)"""
    rng = np.random.default_rng(seed)
    shp = () if B is None else (B,)
    yc = np.concatenate(([g.yg[0]], g.ym, [g.yg[-1]]))
    U = (1.5 * yc * (2 - yc))[None, :, None] * np.ones(shp + (g.Nx, g.Ny + 1, g.Nz)) + noise * rng.standard_normal(shp + (g.Nx, g.Ny + 1, g.Nz))
    V = noise * rng.standard_normal(shp + (g.Nx, g.Ny, g.Nz))
    W = noise * rng.standard_normal(shp + (g.Nx, g.Ny + 1, g.Nz))
    return U, V, W


def rel(a, b):
    a, b = np.asarray(a), np.asarray(b)
    n = np.linalg.norm(b)
    return float(np.linalg.norm(a - b) / n) if n > 0 else float(np.linalg.norm(a - b))
