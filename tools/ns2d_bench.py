"""Measurements of NSControlEnv2D on the engine (GPU box) beside the numpy restatement on the same host.

  python tools/ns2d_bench.py [--out FILE]          ms per env.step at B = 1, 8, 64, 256 with fix_flow on and off (seeded start,
                                                   Re = 3000, opposition control), and the numpy restatement of the same step
  python tools/ns2d_bench.py --profile-only B      20 steps with fix_flow on and 20 with it off and nothing else: the body of a
                                                   `rocprofv3 --kernel-trace --stats` run, a run of its own
Method: warm-up, then 7 timed blocks of `--steps` control steps between two device synchronises, each from the same saved state;
the median, min and max.  A control step is one capped solve (3 solver steps), with fix_flow the bisection (two bracket solves
and about eight more, each run to convergence) and the diagnostics; the step counts of a block are printed beside its time."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pde_policylearning_amd.libs.envs.ns_control_2d import NSControlEnv2D               # noqa: E402
from tests import ns2d_cases as N                                                       # noqa: E402


def make_env(B, fix, dev):
    np.random.seed(0)
    return NSControlEnv2D(argparse.Namespace(fix_flow=fix, Re=3000), detect_plane=-10, bc_type="original", ensemble=B, device=dev)


def gpu_blocks(B, fix, dev, steps, reps=7):
    env = make_env(B, fix, dev)
    for _ in range(3):                                      # past the first step, which sets the target flow
        env.step(env.gt_control())
    start = env.get_state()
    keep = (env.init_bulk_v.clone(), env.info_init)
    out, solver_steps = [], 0
    for r in range(reps + 1):                               # block 0 is the warm-up
        env.set_state(start)
        env.init_bulk_v, env.info_init = keep[0].clone(), keep[1]
        torch.cuda.synchronize()
        t, solver_steps = time.perf_counter(), 0
        for _ in range(steps):
            env.step(env.gt_control())
            solver_steps += int(env.last_steps.max()) + (int(env.last_fixed[:, 4].max()) if fix else 0)
        torch.cuda.synchronize()
        if r:
            out.append((time.perf_counter() - t) / steps * 1e3)
    return statistics.median(out), min(out), max(out), solver_steps / steps


def numpy_blocks(fix, steps, reps=3):
    np.random.seed(0)
    env = N.Restated(3000, fix)
    for _ in range(3):
        env.step(env.gt_control())
    out = []
    for _ in range(reps):
        t, n0 = time.perf_counter(), len(env.fixed)
        for _ in range(steps):
            env.step(env.gt_control())
        out.append((time.perf_counter() - t) / steps * 1e3)
        solver = 3 + (sum(f["steps"] for f in env.fixed[n0:]) / steps if fix else 0)
    return statistics.median(out), min(out), max(out), solver


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--profile-only", type=int, default=0, metavar="B")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    if a.profile_only:
        for fix in (True, False):
            env = make_env(a.profile_only, fix, dev)
            for _ in range(20):
                env.step(env.gt_control())
        torch.cuda.synchronize()
        return
    lines = [f"NSControlEnv2D, 41 x 41, Re = 3000, opposition control; ms per env.step, median [min, max] of 7 blocks of {a.steps} steps;",
             "solver steps = steps of the longest environment per control step (the capped solve and every solve of the bisection)"]

    def say(s):
        print(s, flush=True)
        lines.append(s)
    for fix in (False, True):
        for B in (1, 8, 64, 256):
            med, lo, hi, ss = gpu_blocks(B, fix, dev, a.steps)
            say(f"engine  fix_flow {str(fix):5s} B {B:4d}   {med:9.3f} ms [{lo:.3f}, {hi:.3f}]   {med / B * 1e3:10.1f} us per environment   "
                f"{ss:7.1f} solver steps   {med / ss * 1e3:8.2f} us per solver step")
    for fix in (False, True):
        med, lo, hi, ss = numpy_blocks(fix, max(2, a.steps // 3))
        say(f"numpy   fix_flow {str(fix):5s} B    1   {med:9.3f} ms [{lo:.3f}, {hi:.3f}]   {ss:7.1f} solver steps   {med / ss:8.3f} ms per solver step "
            "(this host's CPU, one environment)")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
