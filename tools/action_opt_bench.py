"""Measurements of the optimal-observer policy (control.OptimalObserverPolicy) at the shipped observer shape: PINObserverFullField
with layers [64] * 5, 12 modes, 3 planes on a 32 x 32 plane, environment 32 x 130 x 32 (GPU box).

  python tools/action_opt_bench.py [--out FILE]            every step below as a child process under its own `timeout`, in order,
                                                           stopping at the first that fails
  python tools/action_opt_bench.py --cell B [--out FILE]   ms per control iteration at B environments, four versions (below),
                                                           alternating blocks
  python tools/action_opt_bench.py --launches [--out FILE] engine launches per epoch of the three eager versions, from the
                                                           library's launch log
  python tools/action_opt_bench.py --profile-only reference|frozen|engine
                                                           5 iterations at B = 1 and nothing else: the body of a
                                                           `rocprofv3 --kernel-trace --stats` run (every dispatch, torch's included)
Versions, EVERY ONE ON ITS OWN COPY of the observer (OptimalObserverPolicy.bind freezes the module it is given):
  reference  the policy composed from the observer's public forward, NormalizerGivenMeanStd.cuda_encode / cuda_decode, torch.norm
             and torch.optim.Adam, as the reference runs it: the observer's parameters keep requires_grad and collect .grad that
             nothing reads, and the observer's front runs as torch ops under the differentiable input, as it did before the
             lifting kernels produced an input gradient (functional.lifting_supported is answered False for this version's
             forward only).  This is what the same composition costs on a checkout without this policy.
  frozen     the same composition with the observer in eval() and its parameters frozen, and the engine front with
             fno_lifting_backward_dx: what is left for the four fno_ctrl_action_* kernels to gain
  eager      control.OptimalObserverPolicy on ControlLoop
  graph      the same as one graph
Method: warm-up, then 7 timed blocks between two device synchronises, each from the same saved state, the versions taking turns
inside every repetition; the median, min and max."""
import argparse
import copy
import os
import statistics
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pde_policylearning_amd import _lib, functional as F                                # noqa: E402
from pde_policylearning_amd.control import ControlLoop, Policy                          # noqa: E402
from pde_policylearning_amd.libs.envs.control_env import ChannelFlowEnv                 # noqa: E402
from pde_policylearning_amd.libs.models.pino_models import PINObserverFullField         # noqa: E402
from pde_policylearning_amd.libs.utilities3 import NormalizerGivenMeanStd               # noqa: E402
from tests import chanflow_step_reference as R                                          # noqa: E402

DT, PLANE, EPOCHS = 1e-3, 10, 10
STEP_TIMEOUT = 240            # seconds per child step


def make_env(B, dev):
    g = R.Grid(32, 130, 32)
    U, V, W = R.analytic_state(g, 1, noise=0.05, B=B)
    return ChannelFlowEnv(g.Nx, g.Nz, g.dx, g.dz, g.y, g.ym, U, V, W, dt=DT, detect_plane=PLANE, device=dev)


def norm():
    rng = np.random.default_rng(0)
    return NormalizerGivenMeanStd(0.05 * rng.standard_normal((32, 32)), 0.2 + 0.1 * rng.random((32, 32)))


def observer(dev):
    torch.manual_seed(0)
    return PINObserverFullField(plane_num=3, modes1=[12] * 4, modes2=[12] * 4, modes3=[12] * 4, fc_dim=128, layers=[64] * 5, in_dim=1,
                                out_dim=1, act="gelu", pad_ratio=[0.0, 0.0625]).to(dev).eval()


class ComposedPolicy(Policy):
    """run_control.py:186-224 from public pieces, every environment with its own norms (the sum of the per-environment losses
    has the per-environment gradients; Adam is elementwise)"""
    name = "optimal-observer (composed)"

    def __init__(self, observer, norm, frozen, epochs=EPOCHS, lr=1e-3, reg_weight=0.1):
        self.observer, self.norm, self.frozen, self.epochs, self.lr, self.reg = observer, norm, frozen, epochs, lr, reg_weight

    def bind(self, env):
        super().bind(env)
        for prm in self.observer.parameters():
            prm.requires_grad_(not self.frozen)
        self.re = torch.full((env.B,), float(getattr(env, "Re", -1.0)), dtype=torch.float32, device=env.device)
        return self

    def act(self, p2):
        env, d, B = self.env, self.env.detect_plane, self.env.B
        torch.neg(env.V[:, :, d, :], out=self.opV1)
        a = (-env.V[:, :, -d, :]).float().requires_grad_(True)
        opt = torch.optim.Adam([a], lr=self.lr)
        with torch.enable_grad():
            for _ in range(self.epochs):
                opt.zero_grad()
                x = self.norm.cuda_encode(a).float()[..., None, None]
                y = self._forward(x)
                field = torch.stack([self.norm.cuda_decode(y[:, k, :, :, 0]) for k in range(y.shape[1])], dim=2)
                loss = (torch.norm(field.reshape(B, -1), dim=1) + self.reg * torch.norm(a.reshape(B, -1), dim=1)).sum()
                loss.backward()
                opt.step()
        a64 = a.detach().double()
        torch.sub(a64, a64.mean(dim=(1, 2), keepdim=True), out=self.opV2)
        return self.opV1, self.opV2

    def _forward(self, x):
        if self.frozen:
            return self.observer(x, self.re)
        saved = F.lifting_supported             # the front as torch ops, as before the lifting had an input gradient
        F.lifting_supported = lambda *a, **k: False
        try:
            return self.observer(x, self.re)
        finally:
            F.lifting_supported = saved


def engine_policy(model):
    from pde_policylearning_amd.control import OptimalObserverPolicy
    return OptimalObserverPolicy(model, norm(), epochs=EPOCHS)


def make_steps(B, dev, which):
    """name -> (step callable, state tensors, loop) of the requested versions, each on its own environment and its own copy
    of the observer"""
    proto = observer(dev)
    out = {}
    for name in which:
        env = make_env(B, dev)
        model = copy.deepcopy(proto)
        pol = ComposedPolicy(model, norm(), frozen=(name == "frozen")) if name in ("reference", "frozen") else engine_policy(model)
        loop = ControlLoop(env, pol, 1, graph=(name == "graph"), explode_at=None)
        loop.observe()
        step = (lambda loop=loop: loop._replay()) if name == "graph" else (lambda loop=loop: loop._iteration(loop.log[0], False))
        out[name] = (step, [env.U, env.V, env.W, env.dPdx_dev], loop)
    return out


def cell(B, dev, say, steps, reps):
    names = ("reference", "frozen", "eager", "graph")
    runs = make_steps(B, dev, names)
    saved = {n: [t.clone() for t in runs[n][1]] for n in names}
    for n in names:                      # warm-up: code objects, the graph capture, the allocator
        for _ in range(5):
            runs[n][0]()
    torch.cuda.synchronize()
    times = {n: [] for n in names}
    for _ in range(reps):
        for n in names:                  # the versions take turns inside every repetition
            for t, s0 in zip(runs[n][1], saved[n]):
                t.copy_(s0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                runs[n][0]()
            torch.cuda.synchronize()
            times[n].append((time.perf_counter() - t0) / steps * 1e3)
    med = statistics.median
    label = {"reference": "composed as the reference (unfrozen, torch front)", "frozen": "composed, frozen observer, engine front",
             "eager": "engine eager", "graph": "engine graph"}
    say(f"B={B:2d}  " + "   ".join(f"{label[n]} {med(times[n]):8.3f} ms (min {min(times[n]):.3f}, max {max(times[n]):.3f})" for n in names))
    r, f, e, g = (med(times[n]) for n in names)
    say(f"B={B:2d}  reference / frozen {r / f:.2f}x   frozen / eager {f / e:.2f}x   eager / graph {e / g:.2f}x   reference / graph {r / g:.2f}x"
        f"   [{steps} iterations x {reps} blocks, {EPOCHS} epochs per iteration]")
    # the versions computed the same thing: opV2 of the last iteration, relative to the engine's
    de = runs["eager"][2].policy.opV2
    for n in ("reference", "frozen"):
        dc = runs[n][2].policy.opV2
        say(f"B={B:2d}  |opV2 {n} - opV2 engine| / |opV2| at the last of the same {steps} iterations from the same state: "
            f"{float((dc - de).norm() / de.norm()):.3e}")


def launches(dev, say):
    from collections import Counter
    for name in ("reference", "frozen", "eager"):
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
    ap.add_argument("--profile-only", default=None, choices=("reference", "frozen", "engine"))
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
    assert torch.cuda.is_available(), "the action-optimisation bench needs a GPU"
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
            say(f"optimal-observer control iteration, observer [64] * 5 / 12 modes / 3 planes on 32 x 32, environment 32 x 130 x 32, "
                f"median of {a.reps} blocks from one saved state")
        cell(a.cell, dev, say, a.steps, a.reps)
    if a.launches:
        launches(dev, say)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
