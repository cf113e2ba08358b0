"""What the step tail (RNO cell gates, fused decode + LpLoss.rel, fused Adam) is held to: the case tables, the float64 /
float32 torch references, the one comparison, and the error table.  Shared by tests/test_step_tail_gpu.py (the HIP kernels
on the GPU) and tests/test_step_tail_reference.py (the same cases and the same comparison on the CPU, with a float32
restatement of each kernel's arithmetic standing in for the engine - and with three planted faults that must be rejected).

Criterion (tests/judging.py::accept, the float32-budget rule): with err = relative L2 against plain torch in float64 on float64
copies of the same float32 inputs,   err_engine == 0 or err_engine < max(floor, BUDGET_SLACK * err_ref32),   err_ref32 being the
error of the same torch expressions in float32.  Floors: 2e-6 gate fields, 2e-5 the four scalar-bias gradients, 1e-5 loss value
and gradient, none for Adam's p / exp_avg / exp_avg_sq.  The exact results the rule's first clause is there for: an all-zero
gradient without weight decay, a bias gradient with h = 0.

Adam at n <= 5 runs ADAM_TINY_K independent instances of the n-element problem (the engine once per instance, each in its
own 8-float slot of the buffers) and pools them into one error: with no floor, the ratio of two float32 roundings of one to
five numbers is a coin toss, the ratio over 256 draws of them is not; every element still goes through the n < 4 / n & 3
path, and the slots' padding must come back untouched."""
import itertools
import math

import torch

from tests.judging import RowLog, accept, rel_err  # noqa: F401  (re-exported to the tests)

FLOOR_GATE, FLOOR_GATE_BIAS, FLOOR_LOSS, FLOOR_ADAM = 2e-6, 2e-5, 1e-5, 0.0
ROWS = RowLog("STEP_TAIL_ERROR_LOG")         # names a file: one line per (case, tensor) appended to it


def judge(case, tensor, err_engine, err_ref32, floor, who="engine"):
    """Record one row of the error table (appended to the file $STEP_TAIL_ERROR_LOG names) and return a description of the
    failure, or None.  Callers collect the failures of a case and assert once, so that every row of the case is recorded."""
    ok = accept(err_engine, err_ref32, floor)
    ROWS.row(case, tensor, who, err_engine, err_ref32, f"floor {floor:7.1e}", "ok" if ok else "FAIL")
    return None if ok else f"{case} {tensor}: {who} {err_engine:.3e}, float32 reference {err_ref32:.3e}, floor {floor:.1e}"


def judge_all(case, got, ref32, ref64, floor_of, who="engine"):
    """every tensor of `ref64` (name -> float64 tensor): got / ref32 hold the same names"""
    bad = []
    for k, r in ref64.items():
        bad.append(judge(case, k, rel_err(got[k], r), rel_err(ref32[k], r), floor_of(k), who))
    return [b for b in bad if b]


def _gen(dev, seed):
    return torch.Generator(device=dev).manual_seed(seed)


# ---------------------------------------------------------------------------------------------------------------------
# RNO cell gates (k_rno_gates.h): rh = sigmoid(a3 + a4 + b2) h;  h' = (1 - sigmoid(a1 + a2 + b1)) h + sigmoid(a7 + a8 + b4) selu(a5 + a6 + b3)
# ---------------------------------------------------------------------------------------------------------------------
GATE_SWEEP = 2048 * 256 * 4                 # elements one trip of the gates' grid-stride loop covers (fno_abi.hip kGateGrid)
GATE_FIELDS = ("a1", "a2", "a7", "a8", "a5", "a6", "a3", "a4", "h")
GATE_BIASES = ("b1", "b4", "b3", "b2")
GATE_PRE = {"r": ("a3", "a4"), "z": ("a1", "a2"), "z2": ("a7", "a8"), "selu": ("a5", "a6")}
SELU_ALPHA, SELU_SCALE = 1.6732632423543772848170429916717, 1.0507009873554804934193349852946


def gate_cases():
    """dicts: name, shape, sigma (common scale: of the four pre-activations a + a' + b and of h), h_zero, sat
    (pre-activation name, sign) or None, noncontig, big (too large for the CPU module)"""
    out = []
    for sigma, h_zero in itertools.product((1e-3, 1e-2, 1e-1, 1.0, 10.0), (False, True)):
        out.append(dict(name=f"gates sigma={sigma:g} h={'0' if h_zero else 'rand'}", shape=(16384,), sigma=sigma, h_zero=h_zero))
    for pre, sign in itertools.product(GATE_PRE, (1.0, -1.0)):
        out.append(dict(name=f"gates saturated {pre} N({sign * 30:+.0f},1)", shape=(16384,), sat=(pre, sign)))
    for n in (4, 1020, GATE_SWEEP, GATE_SWEEP + 4, 3 * GATE_SWEEP - 252):
        out.append(dict(name=f"gates n={n}", shape=(n,), big=n > GATE_SWEEP + 4))
    out.append(dict(name="gates 32x64x128x128", shape=(32, 64, 128, 128), big=True))
    out.append(dict(name="gates non-contiguous a5", shape=(2, 8, 12, 10), noncontig=True))
    for c in out:
        for k, v in (("sigma", 1.0), ("h_zero", False), ("sat", None), ("noncontig", False), ("big", False)):
            c.setdefault(k, v)
    return out


def gate_inputs(case, dev, seed=9):
    """float32 inputs: ({field or bias name: tensor}, upstream gradient of h', upstream gradient of rh)"""
    g, shape, sig = _gen(dev, seed), case["shape"], case["sigma"]
    # the two summands N(0, sigma^2 / 2) each, the scalar bias a quarter sigma: pre-activations of scale sigma around it
    t = {k: (sig if k == "h" else sig * math.sqrt(0.5)) * torch.randn(shape, generator=g, device=dev) for k in GATE_FIELDS}
    t.update({k: 0.25 * sig * torch.randn((), generator=g, device=dev) for k in GATE_BIASES})
    if case["h_zero"]:
        t["h"].zero_()
    if case["sat"]:
        pre, sign = case["sat"]
        for k in GATE_PRE[pre]:                     # the two summands: N(+-15, 1/2) each, so that the sum is N(+-30, 1)
            t[k] = sign * 15.0 + math.sqrt(0.5) * torch.randn(shape, generator=g, device=dev)
    if case["noncontig"]:
        swapped = shape[:-2] + (shape[-1], shape[-2])
        t["a5"] = (sig * math.sqrt(0.5) * torch.randn(swapped, generator=g, device=dev)).transpose(-1, -2)
        assert not t["a5"].is_contiguous() and not torch.isnan(t["a5"]).any()
    g_hn = torch.randn(shape, generator=g, device=dev)
    g_rh = torch.randn(shape, generator=g, device=dev)
    return t, g_hn, g_rh


def gate_outputs(leaves, rh, hn, g_hn, g_rh):
    torch.autograd.backward([hn, rh], [g_hn, g_rh])
    out = {"rh": rh.detach(), "hn": hn.detach()}
    out.update({"d_" + k: leaves[k].grad for k in GATE_FIELDS + GATE_BIASES})
    return out


def gates_torch(t, g_hn, g_rh, dtype):
    """torch.sigmoid / torch.selu under autograd, in `dtype`, on copies of the float32 inputs"""
    v = {k: x.detach().to(dtype).clone().requires_grad_(True) for k, x in t.items()}
    r = torch.sigmoid(v["a3"] + v["a4"] + v["b2"])
    z, z2 = torch.sigmoid(v["a1"] + v["a2"] + v["b1"]), torch.sigmoid(v["a7"] + v["a8"] + v["b4"])
    hn = (1. - z) * v["h"] + z2 * torch.nn.functional.selu(v["a5"] + v["a6"] + v["b3"])
    return gate_outputs(v, r * v["h"], hn, g_hn.to(dtype), g_rh.to(dtype))


def gates_restated(t, g_hn, g_rh, fault=False):
    """The four gate kernels' arithmetic in float32 torch (k_rno_gates.h: values, hand-written gradients, bias gradients
    summed in double).  fault: the negative SELU branch as alpha (exp(s) - 1) forward and alpha exp(s) - alpha backward."""
    f = {k: x.detach().contiguous() for k, x in t.items()}
    A, S = SELU_ALPHA, SELU_SCALE

    def sig(x):
        return 1.0 / (1.0 + torch.exp(-x))

    def selu(s, form):
        neg = {"expm1": lambda: A * torch.expm1(s), "fwd": lambda: A * (torch.exp(s) - 1.0), "bwd": lambda: A * torch.exp(s) - A}[form]()
        return S * torch.where(s > 0, s, neg)
    h = f["h"]
    r = sig(f["a3"] + f["a4"] + f["b2"])
    z, z2, s3 = sig(f["a1"] + f["a2"] + f["b1"]), sig(f["a7"] + f["a8"] + f["b4"]), f["a5"] + f["a6"] + f["b3"]
    out = {"rh": r * h, "hn": (1.0 - z) * h + z2 * selu(s3, "fwd" if fault else "expm1")}
    ds = g_rh * h * r * (1.0 - r)
    dsel = S * torch.where(s3 > 0, torch.ones_like(s3), A * torch.exp(s3))
    d1, d7, d3 = -g_hn * h * z * (1.0 - z), g_hn * selu(s3, "bwd" if fault else "expm1") * z2 * (1.0 - z2), g_hn * z2 * dsel
    out.update(d_a1=d1, d_a2=d1, d_a7=d7, d_a8=d7, d_a5=d3, d_a6=d3, d_a3=ds, d_a4=ds, d_h=g_hn * (1.0 - z) + g_rh * r)
    for k, d in (("d_b1", d1), ("d_b4", d7), ("d_b3", d3), ("d_b2", ds)):
        out[k] = d.double().sum().float()
    return out


def gate_floor(name):
    return FLOOR_GATE_BIAS if name.startswith("d_b") else FLOOR_GATE


# ---------------------------------------------------------------------------------------------------------------------
# fused decode + LpLoss.rel (k_train.h: k_lploss_partial / k_lploss_finish / k_lploss_grad)
# ---------------------------------------------------------------------------------------------------------------------
LOSS_EPS = 1e-5                             # NormalizerGivenMeanStd's eps


def loss_cases():
    """dicts: name, B, n, stats (none / scalar / plane), size_average, gout (upstream gradient scalar), mean_ratio
    (|mean| / std of the raw target)"""
    out = []
    for i, n in enumerate((1, 3, 255, 4096, 4097, 16384, 262144, 128 * 128 * 65)):
        for j, stats in enumerate(("none", "scalar", "plane")):
            out.append(dict(B=4, n=n, stats=stats, size_average=bool((i + j) % 2)))
    for B, stats, sa in itertools.product((1, 257, 1000), ("none", "scalar", "plane"), (False, True)):
        out.append(dict(B=B, n=4097, stats=stats, size_average=sa))
    for stats in ("none", "plane"):
        out.append(dict(B=4, n=4097, stats=stats, size_average=False, gout=-2.5))
    for stats in ("none", "scalar", "plane"):
        out.append(dict(B=4, n=4097, stats=stats, size_average=True, mean_ratio=1e3))
    for c in out:
        c.setdefault("gout", None)
        c.setdefault("mean_ratio", 0.0)
        c["name"] = (f"lploss B={c['B']} n={c['n']} {c['stats']} {'mean' if c['size_average'] else 'sum'}"
                     + (f" gout={c['gout']}" if c["gout"] is not None else "")
                     + (f" mean/std={c['mean_ratio']:g}" if c["mean_ratio"] else ""))
    return out


def loss_inputs(case, dev, seed=5):
    """float32 (pred, target, mean, std): (B, n) fields, statistics None / 0-dim / (n,)"""
    g, B, n = _gen(dev, seed), case["B"], case["n"]
    tgt = case["mean_ratio"] + torch.randn(B, n, generator=g, device=dev)
    pred = tgt + torch.randn(B, n, generator=g, device=dev) * (0.1 if case["mean_ratio"] else 1.0)
    mean = std = None
    if case["stats"] == "scalar":
        mean, std = torch.tensor(0.37, device=dev), torch.tensor(1.9, device=dev)
    elif case["stats"] == "plane":
        mean = torch.randn(n, generator=g, device=dev)
        std = torch.rand(n, generator=g, device=dev) + 0.5
    return pred, tgt, mean, std


def loss_torch(case, pred, tgt, mean, std, dtype):
    """decode + torch.norm (libs/utilities3.py:115-129, 323-334) under autograd, in `dtype`"""
    x = pred.detach().to(dtype).clone().requires_grad_(True)
    y = tgt.to(dtype)
    a, b = (x, y) if std is None else (x * (std.to(dtype) + LOSS_EPS) + mean.to(dtype), y * (std.to(dtype) + LOSS_EPS) + mean.to(dtype))
    ratio = torch.norm(a - b, 2, 1) / torch.norm(b, 2, 1)
    loss = ratio.mean() if case["size_average"] else ratio.sum()
    (loss if case["gout"] is None else loss * case["gout"]).backward()
    return {"loss": loss.detach(), "dpred": x.grad}


def loss_restated(case, pred, tgt, mean, std, drop_from=None):
    """The three loss kernels' arithmetic in float32 torch: squared norms of the decoded difference and target, dn / yn
    summed, coef = scale / (dn * yn) (one product of two norms), gradient = gout * coef * (pred - tgt) * (std + eps)^2.
    drop_from: the planted fault - samples with that index and above are left out of the loss and get a zero coefficient."""
    B = pred.shape[0]
    sc = torch.ones((), device=pred.device) if std is None else std + torch.tensor(LOSS_EPS, dtype=torch.float32, device=pred.device)
    mu = torch.zeros((), device=pred.device) if mean is None else mean
    td = tgt * sc + mu
    d = (pred * sc + mu) - td
    dn, yn = torch.sqrt((d * d).sum(1)), torch.sqrt((td * td).sum(1))
    scale = torch.tensor(1.0 / B if case["size_average"] else 1.0, dtype=torch.float32, device=pred.device)
    coef = torch.where(dn > 0, scale / (dn * yn), torch.zeros_like(dn))
    ratio = dn / yn
    if drop_from is not None:
        ratio, coef = ratio[:drop_from], torch.cat([coef[:drop_from], torch.zeros_like(coef[drop_from:])])
    k = coef * (1.0 if case["gout"] is None else torch.tensor(case["gout"], dtype=torch.float32, device=pred.device))
    return {"loss": scale * ratio.sum(), "dpred": k[:, None] * (pred - tgt) * sc * sc}


SCALE_POWERS = (-20, -8, 8, 20)


def scale_property_inputs(dev, seed=21):
    """(pred, target) for the exact property: with no decoder, (2^k pred, 2^k target) gives the same loss bit for bit and a
    gradient that is exactly 2^-k times the unscaled one - every operation of the three kernels commutes with a power of
    two until something under- or overflows.  The data is checked to do neither in float32 at every k: no squared difference
    or squared target, scaled, is zero, subnormal or infinite, nor are the sums."""
    g = _gen(dev, seed)
    tgt = torch.randn(5, 4097, generator=g, device=dev)
    pred = tgt + torch.randn(5, 4097, generator=g, device=dev)
    tiny = torch.finfo(torch.float32).tiny
    for k in SCALE_POWERS + (0,):
        s = 2.0 ** k
        for sq in (((pred - tgt) * s) ** 2, (tgt * s) ** 2):
            assert float(sq.min()) >= tiny and math.isfinite(float(sq.sum(1).max())), k
        dn, yn = torch.sqrt((((pred - tgt) * s) ** 2).sum(1)), torch.sqrt(((tgt * s) ** 2).sum(1))
        coef = 1.0 / (dn * yn)
        assert float(coef.min()) >= tiny and math.isfinite(float(coef.max())), k
        grad = coef[:, None] * ((pred - tgt) * s)
        assert float(grad.abs().min()) >= tiny and math.isfinite(float(grad.abs().max())), k
    return pred, tgt


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def scale_property_failures(run, dev):
    """run(pred, target) -> (loss, gradient), float32, no decoder"""
    pred, tgt = scale_property_inputs(dev)
    loss0, grad0 = run(pred, tgt)
    bad = []
    for k in SCALE_POWERS:
        s = 2.0 ** k
        loss, grad = run(pred * s, tgt * s)              # (exact: a power of two times a float32 with room to spare)
        if not same_bits(loss.reshape(1), loss0.reshape(1)):
            bad.append(f"k={k}: loss {float(loss)!r} against {float(loss0)!r}")
        if not same_bits(grad, grad0 * (2.0 ** -k)):
            bad.append(f"k={k}: gradient is not 2^{-k} times the unscaled one in {int((grad != grad0 * 2.0 ** -k).sum())} elements")
    return bad


# ---------------------------------------------------------------------------------------------------------------------
# fused Adam (k_train.h: k_adam, k_adam_prep, k_adam_live) against torch.optim.Adam
# ---------------------------------------------------------------------------------------------------------------------
ADAM_LR, ADAM_BETAS, ADAM_EPS = 1e-3, (0.9, 0.999), 1e-8
ADAM_CHECK_STEPS = (1, 20)
ADAM_TINY_K, ADAM_SLOT = 256, 8             # n <= 5: 256 instances, each in its own 8-float (32-byte) slot


def adam_sweep(n_cu):
    """elements one sweep of k_adam covers: the grid is capped at 8 blocks per compute unit, 256 threads, one float4 each"""
    return 8 * n_cu * 256 * 4


def adam_cases(cpu=False):
    """dicts: name, n (an int, or "S+1" / "2S+7" with S = adam_sweep(compute units): adam_resolve), pscale (|p|), gscale
    (0: an all-zero gradient), wd.  Every n at |p| = 1, unit gradients, weight decay 1e-4; the 2 x 4 x 2 table of parameter
    scale x gradient scale x weight decay at n = 1027 and - on the GPU - at 2 S + 7 (three sweeps and an n & 3 tail).
    cpu: without 2 S + 7."""
    out = [dict(n=n, pscale=1.0, gscale=1.0, wd=1e-4) for n in (1, 2, 3, 5, 1027, "S+1", "2S+7") if not cpu or n != "2S+7"]
    for n in (1027,) if cpu else (1027, "2S+7"):
        for pscale, gscale, wd in itertools.product((1.0, 1e-3), (1e-6, 1.0, 1e3, 0.0), (0.0, 1e-4)):
            c = dict(n=n, pscale=pscale, gscale=gscale, wd=wd)
            if c not in out:
                out.append(c)
    for c in out:
        c["name"] = f"adam n={c['n']} |p|={c['pscale']:g} |g|={c['gscale']:g} wd={c['wd']:g}"
    return out


def adam_resolve(case, n_cu):
    S = adam_sweep(n_cu)
    return dict(case, n={"S+1": S + 1, "2S+7": 2 * S + 7}.get(case["n"], case["n"]))


def adam_inputs(case, dev, seed=11):
    """(p0, grad_of): p0 float32 of n elements (n <= 5: ADAM_TINY_K x n), |p0| in [0.5, 1.5) pscale with random signs;
    grad_of(t) the float32 gradient of step t = 1, 2, ...: one unit draw, rotated and rescaled step by step"""
    g, n = _gen(dev, seed), case["n"]
    shape = (ADAM_TINY_K, n) if n <= 5 else (n,)
    mag = 0.5 + torch.rand(shape, generator=g, device=dev)
    p0 = case["pscale"] * torch.where(torch.rand(shape, generator=g, device=dev) < 0.5, -mag, mag)
    base = torch.randn(shape, generator=g, device=dev)

    def grad_of(t):
        return (case["gscale"] * (0.5 + 0.25 * (t % 7))) * base.roll(17 * t, dims=-1)
    return p0, grad_of


def adam_torch(case, p0, grad_of, dtype, steps=ADAM_CHECK_STEPS, state=None, lr=ADAM_LR):
    """torch.optim.Adam in `dtype` on a copy of the float32 parameters; {step: {"p", "exp_avg", "exp_avg_sq"}}.  state:
    (steps already taken, exp_avg, exp_avg_sq) to start from."""
    p = torch.nn.Parameter(p0.detach().to(dtype).clone())
    opt = torch.optim.Adam([p], lr=lr, betas=ADAM_BETAS, eps=ADAM_EPS, weight_decay=case["wd"])
    if state is not None:
        opt.state[p] = dict(step=torch.tensor(float(state[0])), exp_avg=state[1].to(dtype).clone(), exp_avg_sq=state[2].to(dtype).clone())
    out = {}
    for t in range(1, max(steps) + 1):
        p.grad = grad_of(t).to(dtype)
        opt.step()
        if t in steps:
            st = opt.state[p]
            out[t] = {"p": p.detach().clone(), "exp_avg": st["exp_avg"].clone(), "exp_avg_sq": st["exp_avg_sq"].clone()}
    return out


def adam_restated(case, p0, grad_of, steps=ADAM_CHECK_STEPS, bias_step_shift=0):
    """k_adam's arithmetic (adam4) in float32 torch, without the fused multiply-adds: hyperparameters and the two
    bias-correction scalars formed in double and rounded once.  bias_step_shift = -1: the planted fault - the bias
    corrections of step t - 1 (from the second step on: the first would divide by 1 - beta^0)."""
    f32 = lambda x: torch.tensor(x, dtype=torch.float32, device=p0.device)      # noqa: E731
    b1, b2 = ADAM_BETAS
    p, m, v = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
    out = {}
    for t in range(1, max(steps) + 1):
        tb = max(t + bias_step_shift, 1)
        step_size, bc2_sqrt = f32(ADAM_LR / (1.0 - b1 ** tb)), f32(math.sqrt(1.0 - b2 ** tb))
        gg = f32(case["wd"]) * p + grad_of(t)
        m = m + (gg - m) * f32(1.0 - b1)
        v = f32(b2) * v + (gg * gg) * f32(1.0 - b2)
        p = p - step_size * (m / (torch.sqrt(v) / bc2_sqrt + f32(ADAM_EPS)))
        if t in steps:
            out[t] = {"p": p.clone(), "exp_avg": m.clone(), "exp_avg_sq": v.clone()}
    return out


def adam_failures(case, got, ref32, ref64, who="engine"):
    bad = []
    for t in sorted(ref64):
        bad += judge_all(f"{case['name']} step {t}", got[t], ref32[t], ref64[t], lambda k: FLOOR_ADAM, who)
    return bad
