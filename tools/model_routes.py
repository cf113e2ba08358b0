"""Which kernels every model class launches, and the bits it computes, at the smallest shape that reaches each of its routes.
GPU box:  python tools/model_routes.py [--root CHECKOUT] [--out FILE] [--full] [case ...]
          python tools/model_routes.py --compare BASE_RUN_1 BASE_RUN_2 OTHER_RUN

Per case of tests/model_routes_cases.py (of THIS checkout): one seeded forward + backward (loss = sum of squares), then ONE line:
the number of launches, the sha1 of the launch log as `name | variant | grid | block` lines in order, and the sha1 of the bit
image of the output, of the input gradient and of all parameter gradients.  --full prints the launch lines as well (to find
where two runs part).  Only public model classes and _lib.launch_log() are used, and --root names the checkout whose package
runs (default: this one), so the same script records another commit: a refactor of the model layer prints the same file before
and after.

--compare: the cases whose bits differ between two runs of the same commit (atomics, torch's own kernels) are named per field (y, dx, grads)
and held to their launch sequence there; everything else must agree field for field.  Exit status 1 on any difference."""
import argparse
import importlib.util
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))


def load_cases():
    spec = importlib.util.spec_from_file_location("model_routes_cases", os.path.join(os.path.dirname(HERE), "tests", "model_routes_cases.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def record(names, out, full):
    import hashlib
    import torch
    mod = load_cases()
    dev = torch.device("cuda", 0)
    for name in names or mod.CASES:
        try:
            records, sha = mod.run_case(name, mod.CASES[name], dev)
        except (RuntimeError, NotImplementedError, ValueError) as e:
            if "HIP" in str(e) or "hip" in str(e) or "memory access" in str(e):
                raise                      # a device error ends the run: nothing more is started on a GPU that has faulted
            print(f"{name} | refused: {type(e).__name__}: {' '.join(str(e).split())[:200]}", file=out)
            continue
        lines = [f"{r['name']} | {r['variant']} | {r['grid']} | {r['block']}" for r in records]
        log = hashlib.sha1("\n".join(lines).encode()).hexdigest()[:16]
        print(f"{name} | launches {len(lines)} {log} | y {sha['y']} dx {sha['dx']} grads {sha['grads']}", file=out)
        for line in lines if full else ():
            print("    " + line, file=out)
        out.flush()


def parse(path):
    """case -> (launch field, bits field) of a recorded file"""
    return {f[0]: (f[1], f[2] if len(f) > 2 else "") for f in (l.rstrip("\n").split(" | ") for l in open(path) if not l.startswith(" "))}


def compare(base1, base2, other):
    a, b, c = parse(base1), parse(base2), parse(other)
    bad = set(a) != set(b) or set(a) != set(c)
    if bad:
        print("different case lists:", sorted(set(a) ^ set(c)), sorted(set(a) ^ set(b)))
    for name in a:
        if name not in b or name not in c:
            continue
        if a[name][0] != b[name][0]:
            print(f"{name}: the launch sequence differs between the two base runs")
            bad = True
        fa, fb, fc = (dict(zip(v[name][1].split()[::2], v[name][1].split()[1::2])) for v in (a, b, c))
        moving = [k for k in fa if fa[k] != fb.get(k)]
        if moving:
            print(f"{name}: {', '.join(moving)} not bit-stable run to run, held to the launch sequence there")
        if a[name][0] != c[name][0]:
            print(f"{name}: LAUNCH SEQUENCE DIFFERS: {a[name][0]} / {c[name][0]}")
            bad = True
        differ = [k for k in fa if k not in moving and fa[k] != fc.get(k)]
        if differ:
            print(f"{name}: BITS DIFFER: {', '.join(differ)}")
            bad = True
    print(f"{len(a)} cases compared: " + ("DIFFERENCES" if bad else "identical (bit-stable cases bit for bit, the others launch for launch)"))
    return int(bad)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(HERE), help="the checkout whose package runs")
    ap.add_argument("--out", default=None)
    ap.add_argument("--full", action="store_true", help="print every launch line below its case")
    ap.add_argument("--compare", nargs=3, metavar=("BASE1", "BASE2", "OTHER"))
    ap.add_argument("cases", nargs="*")
    args = ap.parse_args()
    if args.compare:
        return compare(*args.compare)
    sys.path.insert(0, os.path.abspath(args.root))
    out = open(args.out, "w") if args.out else sys.stdout
    record(args.cases, out, args.full)
    return 0


if __name__ == "__main__":
    sys.exit(main())
