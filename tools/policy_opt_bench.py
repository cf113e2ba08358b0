"""Measurements of the optimal-policy-observer policy (control.PolicyObserverPolicy) at the shipped shape: PolicyModel2D and
PINObserverFullField (3 planes) both with layers [64] * 5 and 12 modes on a 32 x 32 plane, environment 32 x 130 x 32, three
epochs per control iteration (GPU box).

  python tools/policy_opt_bench.py [--out FILE]            every step below as a child process under its own `timeout`, in order,
                                                           stopping at the first that fails
  python tools/policy_opt_bench.py --cell B [--out FILE]   ms per control iteration at B environments, three versions (below),
                                                           alternating blocks
  python tools/policy_opt_bench.py --launches [--out FILE] engine launches per epoch of the two eager versions, from the
                                                           library's launch log
  python tools/policy_opt_bench.py --profile-only composed|engine|graph
                                                           5 iterations at B = 1 and nothing else: the body of a
                                                           `rocprofv3 --kernel-trace --stats` run (every dispatch, torch's included)
Versions, EVERY ONE ON ITS OWN COPY of both networks (PolicyObserverPolicy.bind freezes the observer and re-points the policy's
parameters at the optimizer's flat buffer):
  composed   the reference's expressions from torch ops around the two modules' public forwards (run_control.py:162-185): the
             observer's parameters keep requires_grad and collect .grad that nothing reads, a NEW torch.optim.Adam over all of
             the policy's parameters per control iteration, torch.norm and loss.backward().  What the same iteration costs
             without this policy class.
  eager      control.PolicyObserverPolicy on ControlLoop
  graph      the same as one graph
Method: warm-up, then 7 timed blocks of 20 iterations between two device synchronises, each from the same saved environment
state, the versions taking turns inside every repetition; the median, min and max."""
import argparse
import copy
import os
import statistics
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pde_policylearning_amd import _lib                                                 # noqa: E402
from pde_policylearning_amd.control import ControlLoop, Policy, PolicyObserverPolicy    # noqa: E402
from pde_policylearning_amd.libs.envs.control_env import ChannelFlowEnv                 # noqa: E402
from pde_policylearning_amd.libs.models.pino_models import PINObserverFullField, PolicyModel2D      # noqa: E402
from tests import chanflow_step_reference as R                                          # noqa: E402

DT, PLANE, EPOCHS, MODES = 1e-3, 10, 3, 12
STEP_TIMEOUT = 300            # seconds per child step
NAMES = ("composed", "eager", "graph")


def make_env(B, dev):
    g = R.Grid(32, 130, 32)
    U, V, W = R.analytic_state(g, 1, noise=0.05, B=B)
    return ChannelFlowEnv(g.Nx, g.Nz, g.dx, g.dz, g.y, g.ym, U, V, W, dt=DT, detect_plane=PLANE, device=dev)


def networks(dev):
    """(policy, observer) at the shipped shape; the policy with the ordinary initialisation and a zero head (zero_init="head"),
    so that every layer carries a gradient, as a trained policy's would"""
    kw = dict(modes1=[MODES] * 4, modes2=[MODES] * 4, modes3=[MODES] * 4, fc_dim=128, layers=[64] * 5, in_dim=1, out_dim=1, act="gelu",
              pad_ratio=[0.0, 0.0625])
    torch.manual_seed(0)
    return PolicyModel2D(zero_init="head", **kw).to(dev), PINObserverFullField(plane_num=3, **kw).to(dev).eval()


class ComposedPolicy(Policy):
    """run_control.py:162-185 from public pieces; the loss of an ensemble is the sum of the environments' own"""
    name = "optimal-policy-observer (composed)"

    def __init__(self, policy_model, observer, epochs=EPOCHS, lr=1e-4, reg_weight=0.1):
        self.policy_model, self.observer, self.epochs, self.lr, self.reg = policy_model, observer, epochs, lr, reg_weight

    def bind(self, env):
        super().bind(env)
        self.re = torch.full((env.B,), float(getattr(env, "Re", -1.0)), dtype=torch.float32, device=env.device)
        return self

    def act(self, p2):
        env, d, B = self.env, self.env.detect_plane, self.env.B
        torch.neg(env.V[:, :, d, :], out=self.opV1)
        a0 = (-env.V[:, :, -d, :]).float()[..., None, None]
        pin = p2.float()[..., None, None]
        opt = torch.optim.Adam(self.policy_model.parameters(), lr=self.lr)
        with torch.enable_grad():
            for _ in range(self.epochs):
                opt.zero_grad()
                x = a0 + self.policy_model(pin, self.re)
                y = self.observer(x, self.re)
                loss = (torch.norm(y.reshape(B, -1), dim=1) + self.reg * torch.norm(x.reshape(B, -1), dim=1)).sum()
                loss.backward()
                opt.step()
        self.opV2.copy_(x.detach().double().reshape(self.opV2.shape))
        return self.opV1, self.opV2


def make_steps(B, dev, which):
    """name -> (step callable, state tensors, loop) of the requested versions, each on its own environment and its own copies
    of the two networks"""
    proto = networks(dev)
    out = {}
    for name in which:
        env = make_env(B, dev)
        pm, obs = copy.deepcopy(proto[0]), copy.deepcopy(proto[1])
        pol = ComposedPolicy(pm, obs) if name == "composed" else PolicyObserverPolicy(pm, obs, epochs=EPOCHS)
        loop = ControlLoop(env, pol, 1, graph=(name == "graph"), explode_at=None)
        loop.observe()
        step = (lambda loop=loop: loop._replay()) if name == "graph" else (lambda loop=loop: loop._iteration(loop.log[0], False))
        out[name] = (step, [env.U, env.V, env.W, env.dPdx_dev], loop)
    return out


def cell(B, dev, say, steps, reps):
    runs = make_steps(B, dev, NAMES)
    saved = {n: [t.clone() for t in runs[n][1]] for n in NAMES}
    for n in NAMES:                      # warm-up: code objects, the graph capture, the allocator
        for _ in range(3):
            runs[n][0]()
    torch.cuda.synchronize()
    times = {n: [] for n in NAMES}
    for _ in range(reps):
        for n in NAMES:                  # the versions take turns inside every repetition
            for t, s0 in zip(runs[n][1], saved[n]):
                t.copy_(s0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                runs[n][0]()
            torch.cuda.synchronize()
            times[n].append((time.perf_counter() - t0) / steps * 1e3)
    med = statistics.median
    label = {"composed": "composed as the reference (unfrozen observer, new torch Adam)", "eager": "engine eager", "graph": "engine graph"}
    say(f"B={B:2d}  " + "   ".join(f"{label[n]} {med(times[n]):8.3f} ms (min {min(times[n]):.3f}, max {max(times[n]):.3f})" for n in NAMES))
    c, e, g = (med(times[n]) for n in NAMES)
    say(f"B={B:2d}  composed / eager {c / e:.2f}x   eager / graph {e / g:.2f}x   composed / graph {c / g:.2f}x"
        f"   [{steps} iterations x {reps} blocks, {EPOCHS} epochs per iteration]")
    losses = runs["eager"][2].policy.losses.cpu()
    say(f"B={B:2d}  engine eager, last iteration: loss per epoch (environment 0) " + ", ".join(f"{float(v):.6f}" for v in losses[:, 0, 0]))


def launches(dev, say):
    from collections import Counter
    for name in ("composed", "eager"):
        step, _, loop = make_steps(1, dev, (name,))[name]
        step()
        with _lib.launch_log() as log:
            step()
        torch.cuda.synchronize()
        n = Counter(r["name"] for r in log.records)
        total = len(log.records)
        env_part = sum(v for k, v in n.items() if "chanflow" in k)
        say(f"{name:9s}: {total} engine launches per control iteration, {env_part} of them the environment step, pressure and diagnostics; "
            f"{(total - env_part) / EPOCHS:.1f} engine launches per epoch (torch's own kernels are not in this log: see the kernel trace)")
        say("          " + ", ".join(f"{k} x{v}" for k, v in sorted(n.items()) if "chanflow" not in k))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--cell", type=int, default=0)
    ap.add_argument("--launches", action="store_true")
    ap.add_argument("--profile-only", default=None, choices=("composed", "engine", "graph"))
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    if not (a.cell or a.launches or a.profile_only):
        # the driver initialises no GPU: every step is a fresh child under its own time limit; a failure ends the run
        tail = ["--out", a.out] if a.out else []
        for args in (["--cell", "1"], ["--cell", "8"], ["--launches"]):
            cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT), sys.executable, os.path.abspath(__file__), "--steps", str(a.steps),
                   "--reps", str(a.reps)] + args + tail
            rc = subprocess.run(cmd).returncode
            if rc != 0:
                print(f"step {' '.join(args)} ended with status {rc}: nothing further is started", flush=True)
                sys.exit(rc)
        return
    assert torch.cuda.is_available(), "the policy-optimisation bench needs a GPU"
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    if a.profile_only:
        name = "eager" if a.profile_only == "engine" else a.profile_only
        step = make_steps(1, dev, (name,))[name][0]
        for _ in range(5):
            step()
        torch.cuda.synchronize()
        return
    if a.cell:
        if a.cell == 1:
            say(f"optimal-policy-observer control iteration, policy and observer [64] * 5 / {MODES} modes on 32 x 32, environment "
                f"32 x 130 x 32, median of {a.reps} blocks from one saved state")
        cell(a.cell, dev, say, a.steps, a.reps)
    if a.launches:
        launches(dev, say)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
