"""Poisoned-buffer and guard-band cases for the control-loop entry points (tests/hygiene.py): outputs and workspaces pre-filled
with 0x00 / 0xFF (NaN) / 0x7F patterns inside guard bands, inputs inside NaN-filled guarded buffers.  Every output is bitwise
equal across the runs and finite, the guard bands are intact, the inputs come back unchanged.

Safety (hygiene.py's rule: poison only data): the bridges read and write planes of floats and doubles, the diagnostics
workspace holds partial sums, the statistics' mean and M2 are doubles; the pointer table of the statistics is a kernel argument
built by the host.  Nothing a kernel turns into an address lives in a poisoned buffer."""
import numpy as np
import pytest
import torch

from tests import chanflow_step_reference as R
from tests import hygiene as H
from tests.judging import dev  # noqa: F401

pytestmark = pytest.mark.gpu
SHAPES = [(6, 7, 10, 1), (8, 10, 6, 3), (32, 130, 32, 2)]


def _planes(dev, Nx, Nz, B):
    rng = np.random.default_rng(Nx * 100 + Nz + B)
    t = lambda a, dt=torch.float64: torch.from_numpy(np.ascontiguousarray(a)).to(dt).to(dev)
    return {"p": t(0.03 * rng.standard_normal((B, Nx, Nz))), "mean": t(0.01 * rng.standard_normal((Nx, Nz))),
            "std": t(0.02 + np.abs(0.01 * rng.standard_normal((Nx, Nz)))), "y": t(rng.standard_normal((B, 3, Nx, Nz)), torch.float32)}


@pytest.mark.parametrize("Nx,Ny,Nz,B", SHAPES)
def test_bridges(dev, Nx, Ny, Nz, B):
    from pde_policylearning_amd import functional as F
    plane = Nx * Nz

    def fn(inp, after_forward):
        dense = F.ctrl_encode(inp["p"], inp["mean"], inp["std"])
        x = F.torch.empty((B, 3, Nx, Nz), dtype=torch.float32, device=dev)          # poisoned while a pattern is active
        F.ctrl_encode(inp["p"], inp["mean"], inp["std"], out=x, batch_stride=3 * plane)
        v1, v2 = F.ctrl_decode(inp["y"], inp["mean"], inp["std"], shape=(B, Nx, Nz), batch_stride=3 * plane, zero_mean=True, clip=0.05)
        w1, w2 = F.ctrl_decode(inp["y"], inp["mean"], inp["std"], shape=(B, Nx, Nz), batch_stride=3 * plane)
        after_forward()
        return {"dense": dense, "x0": x[:, 0], "opV1": v1, "opV2": v2, "plain opV1": w1, "plain opV2": w2}
    H.assert_clean(f"ctrl bridges {Nx}x{Nz} B={B}", fn, _planes(dev, Nx, Nz, B))


@pytest.mark.parametrize("Nx,Ny,Nz,B", SHAPES)
def test_diagnostics2(dev, Nx, Ny, Nz, B):
    from pde_policylearning_amd import functional as F
    g = R.Grid(Nx, Ny, Nz)
    grid = F.ChannelGrid(g.Nx, g.Nz, g.dx, g.dz, g.y, g.ym, g.yg, g.nu)
    poisson = F.ChannelPoisson(grid)
    U, V, W = (torch.from_numpy(a).to(dev) for a in R.analytic_state(g, 7 + B, noise=0.1, B=B))
    inputs = {"U": U, "V": V, "W": W, "p2": _planes(dev, Nx, Nz, B)["p"], "dp": torch.full((B,), R.DPDX0, dtype=torch.float64, device=dev)}

    def fn(inp, after_forward):
        log = F.torch.empty((3, B, 13), dtype=torch.float64, device=dev)
        F.chanflow_diagnostics2(grid, poisson, inp["U"], inp["V"], inp["W"], inp["p2"], inp["dp"], out=log[1])
        none = F.chanflow_diagnostics2(grid, poisson, inp["U"], inp["V"], inp["W"], None, inp["dp"])
        after_forward()
        return {"row": log[1], "without p2": none}
    H.assert_clean(f"chanflow_diagnostics2 {Nx}x{Ny}x{Nz} B={B}", fn, inputs)


@pytest.mark.parametrize("Nx,Ny,Nz,B", SHAPES)
def test_running_stats(dev, Nx, Ny, Nz, B):
    from pde_policylearning_amd import functional as F
    rng = np.random.default_rng(3)
    sizes = [(B, Nx, Nz), (B, Nx, Ny + 1, Nz), (B, Nx, Ny, Nz), (5,)]
    inputs = {f"x{t}.{k}": torch.from_numpy(rng.standard_normal(s)).to(dev) for t in range(3) for k, s in enumerate(sizes)}

    def fn(inp, after_forward):
        means = [F.torch.empty(s, dtype=torch.float64, device=dev) for s in sizes]
        m2s = [F.torch.empty(s, dtype=torch.float64, device=dev) for s in sizes]
        for t in range(3):
            F.running_stats_update([inp[f"x{t}.{k}"] for k in range(len(sizes))], means, m2s, t + 1)
        after_forward()
        out = {f"mean{k}": m for k, m in enumerate(means)}
        out.update({f"m2.{k}": m for k, m in enumerate(m2s)})
        return out
    H.assert_clean(f"running_stats_update {Nx}x{Ny}x{Nz} B={B}", fn, inputs)
