"""ms per environment step (chanflow_rk3_step + chanflow_wall_pressure) at the shipped grid 32 x 130 x 32, eager and as one
graph, for B = 1, 8, 64; the CPU restatement (dense solves) on the same host beside it.
GPU box:  python tools/chanflow_step_bench.py [--out FILE] [--profile-only B]
Method: warm-up, then blocks of many steps between two device synchronises, each from the same saved state, the median of
the blocks; one process.
--profile-only B runs a short eager loop and nothing else: the body of a `rocprofv3 --kernel-trace --stats` run."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pde_policylearning_amd import _lib, functional as F      # noqa: E402
from tests import chanflow_step_reference as R                # noqa: E402

DT, PLANE = 1e-3, 10


def setup(B, dev):
    g = R.Grid(32, 130, 32)
    grid = F.ChannelGrid(g.Nx, g.Nz, g.dx, g.dz, g.y, g.ym, g.yg, g.nu)
    U, V, W = (torch.from_numpy(a).to(dev) for a in R.analytic_state(g, 1, noise=0.05, B=B))
    dp = torch.full((B,), R.DPDX0, dtype=torch.float64, device=dev)
    mu = torch.tensor([R.bulk_velocity(g, U[b].cpu().numpy()) for b in range(B)], dtype=torch.float64, device=dev)
    return g, grid, F.ChannelPoisson(grid), U, V, W, dp, mu


def blocks(step, steps, reps, state):
    """median, min, max ms per step over `reps` timed blocks; every block (and the warm-up) starts from the same saved state,
    so the flow that is timed is the one that was set up, however long the measurement runs"""
    saved = [t.clone() for t in state]

    def restore():
        for t, s0 in zip(state, saved):
            t.copy_(s0)
        torch.cuda.synchronize()
    for _ in range(max(5, steps // 10)):
        step()
    out = []
    for _ in range(reps):
        restore()
        t = time.perf_counter()
        for _ in range(steps):
            step()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t) / steps * 1e3)
    return statistics.median(out), min(out), max(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--profile-only", type=int, default=0)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the step bench needs a GPU"
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    if a.profile_only:
        g, grid, poisson, U, V, W, dp, mu = setup(a.profile_only, dev)
        ws = F.chanflow_step_workspace(grid, a.profile_only, dev)
        v1, v2 = -V[:, :, PLANE, :].contiguous(), -V[:, :, -PLANE, :].contiguous()
        for _ in range(20):
            F.chanflow_rk3_step(grid, poisson, U, V, W, v1, v2, dp, mu, DT, ws=ws)
            p2 = F.chanflow_wall_pressure(grid, poisson, U, V, W, dp, ws=ws)[1]
            F.chanflow_diagnostics(grid, poisson, U, V, W, p2)        # what ChannelFlowEnv.step adds for `info`
        torch.cuda.synchronize()
        return
    say("channel-flow environment step (rk3_step + wall_pressure), 32 x 130 x 32, float64")
    lib = _lib.lib()
    for B in (1, 8, 64):
        g, grid, poisson, U, V, W, dp, mu = setup(B, dev)
        ws = F.chanflow_step_workspace(grid, B, dev)
        p1, p2 = (torch.empty((B, g.Nx, g.Nz), dtype=torch.float64, device=dev) for _ in range(2))
        v1, v2 = -V[:, :, PLANE, :].contiguous(), -V[:, :, -PLANE, :].contiguous()

        def eager():
            F.chanflow_rk3_step(grid, poisson, U, V, W, v1, v2, dp, mu, DT, ws=ws)
            F.chanflow_wall_pressure(grid, poisson, U, V, W, dp, ws=ws, out=(p1, p2))
        if B == 1:
            lib.fno_profile_reset()
            lib.fno_profile_enable(1)
            eager()
            torch.cuda.synchronize()
            rec = _lib.profile_summary()
            lib.fno_profile_enable(0)
            lib.fno_profile_reset()
            say(f"launches per step: {sum(n for _, _, n in rec)}  ({', '.join(f'{k} x{n}' for k, _, n in rec)})")
        steps = max(20, a.steps // max(1, B // 8))
        me, lo, hi = blocks(eager, steps, a.reps, (U, V, W, dp))
        gs = F.GraphedChannelStep(grid, poisson, U, V, W, dp, mu, DT)
        gs.opV1.copy_(v1)
        gs.opV2.copy_(v2)
        mg, lg, hg = blocks(gs.step, steps, a.reps, (gs.U, gs.V, gs.W, gs.dPdx))
        say(f"B={B:3d}  eager {me:8.3f} ms/step (min {lo:.3f}, max {hi:.3f})   graph {mg:8.3f} ms/step (min {lg:.3f}, max {hg:.3f})"
            f"   {me / B:.3f} / {mg / B:.3f} ms per environment   [{a.reps} blocks of {steps} steps]")
        if not all(bool(torch.isfinite(t).all()) for t in (U, V, W, gs.U, gs.p2)):
            say(f"WARNING: B={B}: the state left the finite range during a timed block")
    g = R.Grid(32, 130, 32)
    U0, V0, W0 = R.analytic_state(g, 1)
    v1, v2 = R.gt_control(V0, PLANE)
    m0 = R.bulk_velocity(g, U0)
    t = time.perf_counter()
    Un, Vn, Wn, dpn = R.rk3_step(g, U0, V0, W0, v1, v2, R.DPDX0, m0, DT)
    R.pressure(g, Un, Vn, Wn, dpn)
    say(f"CPU restatement (numpy, dense solves, {torch.get_num_threads()} threads), same host: {(time.perf_counter() - t) * 1e3:.0f} ms per step")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
