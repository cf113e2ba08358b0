"""Generate tests/golden/ns2d_reference.npz by running the reference's own NSControlEnv2D (libs/envs/ns_control_2d.py) on the CPU.

usage: python tools/make_ns2d_golden.py --ref <checkout of the reference> [--out tests/golden/ns2d_reference.npz]

The module imports wandb, matlab.engine and sklearn.metrics at its top and uses none of them in the solver; absent ones are
replaced by oracle.make_golden.install_standins() and a placeholder for sklearn.  `solve` and `solve_fixed_mass` are called on
an object of the class made without its constructor and given exactly the attributes they read, so that grids other than the
constructor's 41 x 41 run too; the environment cases go through the real constructor and `step`.  What is written is data only:
outputs, step counts, bisection counts and info values.  The inputs are the deterministic cases of tests/ns2d_cases.py."""
import argparse
import contextlib
import io
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle.make_golden import install_standins  # noqa: E402
from tests import ns2d_cases as N  # noqa: E402


def reference_module(ref):
    install_standins()
    try:
        import sklearn.metrics  # noqa: F401
    except ImportError:
        sk, skm = types.ModuleType("sklearn"), types.ModuleType("sklearn.metrics")
        skm.mean_squared_error = None
        sk.metrics = skm
        sys.modules.update({"sklearn": sk, "sklearn.metrics": skm})
    sys.path.insert(0, ref)
    from libs.envs import ns_control_2d
    return ns_control_2d


def bare_env(mod, g, state, nu, F):
    env = object.__new__(mod.NSControlEnv2D)
    env.nx, env.ny, env.nit, env.dx, env.dy, env.dt, env.rho, env.nu, env.F = g.nx, g.ny, g.nit, g.dx, g.dy, g.dt, 1, nu, F
    env.p, env.u, env.v = (np.array(a, dtype=np.float64) for a in state)
    return env


def ref_solve(mod, g, state, bc, max_step, nu, F):
    env = bare_env(mod, g, state, nu, F)
    bulk = env.solve(bc, max_step, env.p, env.u, env.v, g.dx, g.dy, g.dt, 1, nu, F, update_state=True)
    return env, bulk


def count_solve_steps(mod):
    """wrap the class's solve so that every call's step count is recorded (it is a local of the method: recount from udiff)"""
    counts = []
    orig = mod.NSControlEnv2D.solve
    real_sum = np.sum

    def solve(self, *a, **k):
        calls = [0]

        def counting_sum(x, *aa, **kk):
            calls[0] += 1
            return real_sum(x, *aa, **kk)
        mod.np.sum = counting_sum
        try:
            out = orig(self, *a, **k)
        finally:
            mod.np.sum = real_sum
        counts.append(calls[0] // 3)                       # udiff (:472) calls np.sum three times per step
        return out
    mod.NSControlEnv2D.solve = solve
    return counts


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--ref", required=True)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "ns2d_reference.npz"))
    a = ap.parse_args()
    mod = reference_module(a.ref)
    counts = count_solve_steps(mod)
    out = {}
    with contextlib.redirect_stdout(io.StringIO()):
        # capped solves, max_step = 3
        for ny, nx in N.CAPPED_GRIDS:
            g = N.Grid(ny, nx)
            states, bcs = N.capped_case(ny, nx)
            for b, (st, bc) in enumerate(zip(states, bcs)):
                del counts[:]
                env, bulk = ref_solve(mod, g, st, bc, 3, N.CAPPED_NU[b], N.CAPPED_F[b])
                tag = f"capped_{ny}x{nx}_{b}"
                out.update({f"{tag}/p": env.p, f"{tag}/u": env.u, f"{tag}/v": env.v, f"{tag}/bulk_v": np.float64(bulk),
                            f"{tag}/steps": np.int64(counts[-1])})
        # converged solves
        for tag, g, st in (("conv_9x12", N.Grid(9, 12), N.small_start()), ("conv_41x41", N.Grid(41, 41), N.seeded_start())):
            del counts[:]
            env, bulk = ref_solve(mod, g, st, None, -1, 1 / 3000, 4.0)
            out.update({f"{tag}/p": env.p, f"{tag}/u": env.u, f"{tag}/v": env.v, f"{tag}/bulk_v": np.float64(bulk),
                        f"{tag}/steps": np.int64(counts[-1])})
        # the environment: seeded start, Re = 3000, six steps of gt_control, fix_flow on and off; the fixed-mass solve on the
        # state after the first control step
        for fix in (True, False):
            np.random.seed(0)
            env = mod.NSControlEnv2D(types.SimpleNamespace(fix_flow=fix, Re=3000), detect_plane=-10, bc_type="original")
            tag = "env_fix" if fix else "env_free"
            infos, forces, bis = [], [], []
            for t in range(6):
                del counts[:]
                _, _, _, info = env.step(env.gt_control(), print_info=False)
                infos.append(info)
                forces.append(env.F)
                bis.append(len(counts) - 3 if fix else 0)          # solves of the step: one capped, two brackets, the bisections
                if t == 0 and not fix:
                    bc = env.gt_control()
                    target = env.cal_bulk_v()
                    del counts[:]
                    r = env.solve_fixed_mass(bc, target, 0, 3 * env.F, verbose=False)
                    out.update({"fixed/result_f": np.float64(r[0]), "fixed/flow": np.float64(r[1]), "fixed/error": np.float64(r[2]),
                                "fixed/bisections": np.int64(len(counts) - 2), "fixed/steps": np.int64(sum(counts)),
                                "fixed/target": np.float64(target)})
            keys = sorted(infos[-1])
            out.update({f"{tag}/p": env.p, f"{tag}/u": env.u, f"{tag}/v": env.v, f"{tag}/F": np.array(forces, dtype=np.float64),
                        f"{tag}/bisections": np.array(bis, dtype=np.int64), f"{tag}/info_keys": np.array(keys),
                        f"{tag}/first_info_keys": np.array(sorted(infos[0])),
                        f"{tag}/infos": np.array([[i.get(k, np.nan) for k in keys] for i in infos], dtype=np.float64)})
    np.savez_compressed(a.out, **out)
    print(f"{a.out}: {len(out)} arrays, {os.path.getsize(a.out)} bytes")


if __name__ == "__main__":
    main()
