"""Measurements of the closed control loop at the shipped grid 32 x 130 x 32 (GPU box).

  python tools/control_loop_bench.py --diag [--out FILE]      the two-level diagnostics beside the one-workgroup kernel: device-event
                                                              time of 20 calls each, 5 alternating blocks, B = 1, 8, 64
  python tools/control_loop_bench.py --iter [--out FILE]      ms per control iteration, eager and graph, GtPolicy and
                                                              FnoPolicy(FNO2dObserver(12, 12, 32)), B = 1, 8, 64, beside the unbridged
                                                              composition on the environment's public API (get_boundary_pressures ->
                                                              host encode -> model -> host decode -> env.step), alternating
  python tools/control_loop_bench.py --profile-only B         20 iterations with both diagnostics and nothing else: the body of a
                                                              `rocprofv3 --kernel-trace --stats` run
Method: warm-up, then 7 timed blocks between two device synchronises, each from the same saved state; the median, min and max."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pde_policylearning_amd import functional as F                                      # noqa: E402
from pde_policylearning_amd.control import ControlLoop, FnoPolicy, GtPolicy             # noqa: E402
from pde_policylearning_amd.libs.envs.control_env import ChannelFlowEnv                 # noqa: E402
from pde_policylearning_amd.libs.models.fno_models import FNO2dObserver                 # noqa: E402
from tests import chanflow_step_reference as R                                          # noqa: E402

DT, PLANE = 1e-3, 10


class Norm:
    def __init__(self, mean, std, eps=1e-5):
        self.mean, self.std, self.eps = mean, std, eps


def make_env(B, dev):
    g = R.Grid(32, 130, 32)
    U, V, W = R.analytic_state(g, 1, noise=0.05, B=B)
    return ChannelFlowEnv(g.Nx, g.Nz, g.dx, g.dz, g.y, g.ym, U, V, W, dt=DT, detect_plane=PLANE, device=dev)


def norms():
    rng = np.random.default_rng(0)
    u, v = rng.standard_normal((32, 32)), rng.standard_normal((32, 32))
    return Norm(0.01 * u, 0.02 + np.abs(0.01 * u)), Norm(0.002 * v, 0.01 + np.abs(0.005 * v))


def blocks(step, steps, reps, state):
    saved = [t.clone() for t in state()]

    def restore():
        for t, s0 in zip(state(), saved):
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


def diag_pair(B, dev, say, calls=20, reps=5):
    env = make_env(B, dev)
    p2 = env.get_boundary_pressures()[1].reshape(B, 32, 32)
    ws = F.chanflow_diagnostics2_workspace(env.grid, B, dev)
    row = torch.zeros((B, 13), dtype=torch.float64, device=dev)
    old = lambda: F.chanflow_diagnostics(env.grid, env.poisson, env.U, env.V, env.W, p2)
    new = lambda: F.chanflow_diagnostics2(env.grid, env.poisson, env.U, env.V, env.W, p2, env.dPdx_dev, out=row, ws=ws)
    res = {"old": [], "new": []}
    for fn in (old, new):
        for _ in range(5):
            fn()
    for _ in range(reps):
        for name, fn in (("old", old), ("new", new)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            for _ in range(calls):
                fn()
            b.record()
            torch.cuda.synchronize()
            res[name].append(a.elapsed_time(b) / calls * 1e3)
    o, n = res["old"], res["new"]
    say(f"B={B:3d}  k_chanflow_diag {statistics.median(o):8.1f} us (min {min(o):.1f}, max {max(o):.1f})   two-level pair "
        f"{statistics.median(n):8.1f} us (min {min(n):.1f}, max {max(n):.1f})   ratio {statistics.median(o) / statistics.median(n):.2f}x"
        "   [device events around 20 back-to-back calls, launch gaps included]")


def unbridged(env, model, p_norm, v_norm, policy):
    """the composition the loop replaces, on the environment's public API"""
    dev = env.device

    def step():
        if policy == "gt":
            env.get_boundary_pressures()
            v1, v2 = env.gt_control()
        else:
            p2 = env.get_boundary_pressures()[1].cpu().numpy().reshape(env.B, 32, 32)
            x = torch.from_numpy(((p2 - p_norm.mean) / (p_norm.std + p_norm.eps)).astype(np.float32)).to(dev)[..., None]
            with torch.no_grad():
                y = model(x).reshape(env.B, 32, 32).cpu().numpy().astype(np.float64)
            v2 = y * (v_norm.std + v_norm.eps) + v_norm.mean
            v2 = torch.from_numpy(v2 - v2.mean(axis=(1, 2), keepdims=True)).to(dev).reshape(env._out(env.U[:, :, 0, :]).shape)
            v1 = torch.zeros_like(v2)
        env.step(v1, v2)
    return step


def iteration_table(dev, say, steps, reps):
    p_norm, v_norm = norms()
    torch.manual_seed(0)
    model = FNO2dObserver(12, 12, 32).to(dev).eval()
    for B in (1, 8, 64):
        for policy in ("gt", "fno"):
            mk = lambda: GtPolicy() if policy == "gt" else FnoPolicy(model, p_norm, v_norm, zero_mean=True)
            cells = {}
            for name in ("unbridged", "eager", "graph"):
                env = make_env(B, dev)
                state = lambda env=env: [env.U, env.V, env.W, env.dPdx_dev]
                if name == "unbridged":
                    step = unbridged(env, model, p_norm, v_norm, policy)
                else:
                    loop = ControlLoop(env, mk(), 1, graph=(name == "graph"))
                    loop.observe()
                    step = (lambda loop=loop: loop._iteration(loop.log[0], False)) if name == "eager" else (lambda loop=loop: loop._replay())
                cells[name] = blocks(step, steps if B < 64 else max(steps // 4, 10), reps, state)
            u, e, gph = cells["unbridged"], cells["eager"], cells["graph"]
            say(f"B={B:3d} {policy:3s}  unbridged {u[0]:8.3f} ms (min {u[1]:.3f}, max {u[2]:.3f})   loop eager {e[0]:8.3f} ms (min {e[1]:.3f}, "
                f"max {e[2]:.3f})   loop graph {gph[0]:8.3f} ms (min {gph[1]:.3f}, max {gph[2]:.3f})   unbridged / eager {u[0] / e[0]:.2f}x   "
                f"unbridged / graph {u[0] / gph[0]:.2f}x")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--diag", action="store_true")
    ap.add_argument("--iter", action="store_true")
    ap.add_argument("--profile-only", type=int, default=0)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the control-loop bench needs a GPU"
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    if a.profile_only:
        B = a.profile_only
        env = make_env(B, dev)
        loop = ControlLoop(env, GtPolicy(), 1)
        loop.observe()
        for _ in range(20):
            loop._iteration(loop.log[0], False)
            F.chanflow_diagnostics(env.grid, env.poisson, env.U, env.V, env.W, loop.p2)      # the one-workgroup kernel beside the pair
        torch.cuda.synchronize()
        return
    if a.diag:
        say("diagnostics at 32 x 130 x 32, float64: k_chanflow_diag (one workgroup per sample) vs k_chanflow_diag_part + _finish")
        for B in (1, 8, 64):
            diag_pair(B, dev, say)
    if a.iter:
        say(f"control iteration at 32 x 130 x 32, float64 state, median of {a.reps} blocks from one saved state")
        iteration_table(dev, say, a.steps, a.reps)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
