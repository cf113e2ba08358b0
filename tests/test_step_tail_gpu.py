"""The streaming kernels around the fused model - RNO cell gates (k_rno_gates.h), fused decode + LpLoss.rel and Adam
(k_train.h) - against plain torch in float64, across sizes (second and later trips of every grid-stride loop, ragged last
trips, scalar tails), magnitudes and saturation.  Cases, references and the comparison: tests/step_tail_cases.py (the
criterion is shown to bite, and to be passable, on the CPU in tests/test_step_tail_reference.py).  Every (case, tensor) adds
a row - engine error, float32-torch error - to the file $STEP_TAIL_ERROR_LOG names (profiles/r10_step_tail_errors.txt).

What the sizes reach:
  gates    one sweep of the fixed 2048 x 256 grid is N = 2 097 152 elements: N (exactly one trip), N + 4 (one thread's second
           trip), 3 N - 252 (a ragged third trip), 32 x 64 x 128 x 128 (BASELINE config 3's state: 16 trips)
  LpLoss   k_lploss_partial gives a sample 16 x 256 threads: n = 4 097 is the first second element of a thread, 1 064 960
           the 260th; k_lploss_finish walks samples 256 at a time: B = 257 / 1 000 are its second / fourth trip;
           k_lploss_grad's grid is capped at 64 x 256 threads: n > 16 384
  Adam     S = 8 blocks per compute unit x 256 threads x 4 elements: S + 1 (second sweep is one scalar-tail element),
           2 S + 7 (three sweeps and a three-element tail); n = 1, 2, 3, 5: the tail alone / beside one float4
           k_adam_live: 8 x CUs x 256 complex pairs a sweep - no case of tests/test_lazy_adam_gpu.py exceeds it, one here does"""
import pytest
import torch

from tests import step_tail_cases as T
from tests.judging import dev  # noqa: F401

pytestmark = pytest.mark.gpu

GATE_CASES, LOSS_CASES, ADAM_CASES = T.gate_cases(), T.loss_cases(), T.adam_cases()


def _ids(cases):
    return [c["name"].replace(" ", "_") for c in cases]


def _n_cu(dev):
    return torch.cuda.get_device_properties(dev).multi_processor_count       # what fno_abi.hip's dev_ncu() reads


# ---------------------------------------------------------------------------------------------------------------------
# gates
# ---------------------------------------------------------------------------------------------------------------------
def _gates_engine(t, g_hn, g_rh):
    from pde_policylearning_amd import functional as F
    v = {k: x.detach().clone().requires_grad_(True) for k, x in t.items()}
    for k in t:
        assert v[k].is_contiguous() == t[k].is_contiguous(), k               # (the copy keeps a permuted operand permuted)
    hn = F.rno_output_gate(v["a1"], v["a2"], v["b1"], v["a7"], v["a8"], v["b4"], v["a5"], v["a6"], v["b3"], v["h"])
    rh = F.rno_reset_gate(v["a3"], v["a4"], v["b2"], v["h"])
    return T.gate_outputs(v, rh, hn, g_hn, g_rh)


@pytest.mark.parametrize("case", GATE_CASES, ids=_ids(GATE_CASES))
def test_gates_vs_float64(dev, case):
    """rno_reset_gate / rno_output_gate: both outputs, the gradient of every field and of the four scalar biases"""
    t, g_hn, g_rh = T.gate_inputs(case, dev)
    got = _gates_engine(t, g_hn, g_rh)
    assert all(torch.isfinite(x).all() for x in got.values())
    ref32 = T.gates_torch(t, g_hn, g_rh, torch.float32)
    ref64 = T.gates_torch(t, g_hn, g_rh, torch.float64)
    bad = T.judge_all(case["name"], got, ref32, ref64, T.gate_floor)
    assert not bad, "\n".join(bad)
    if case["noncontig"]:
        # _operand's copy feeds the same values: the same numbers handed over contiguous give the same bits
        t2 = dict(t, a5=t["a5"].contiguous())
        again = _gates_engine(t2, g_hn, g_rh)
        for k in got:
            assert T.same_bits(got[k].reshape(-1), again[k].reshape(-1)), k


# ---------------------------------------------------------------------------------------------------------------------
# decode + LpLoss.rel
# ---------------------------------------------------------------------------------------------------------------------
def _loss_engine(case, pred, tgt, mean, std):
    from pde_policylearning_amd.trainer import FusedLpLoss, MeanStdDecoder
    dec = None if std is None else MeanStdDecoder(mean, std, eps=T.LOSS_EPS, device=pred.device)
    x = pred.detach().clone().requires_grad_(True)
    loss = FusedLpLoss(size_average=case["size_average"], decoder=dec)(x, tgt)
    (loss if case["gout"] is None else loss * case["gout"]).backward()
    return {"loss": loss.detach(), "dpred": x.grad}


@pytest.mark.parametrize("case", LOSS_CASES, ids=_ids(LOSS_CASES))
def test_lploss_vs_float64(dev, case):
    inp = T.loss_inputs(case, dev)
    got = _loss_engine(case, *inp)
    ref32, ref64 = T.loss_torch(case, *inp, torch.float32), T.loss_torch(case, *inp, torch.float64)
    bad = T.judge_all(case["name"], got, ref32, ref64, lambda k: T.FLOOR_LOSS)
    assert not bad, "\n".join(bad)


def test_lploss_power_of_two_scaling_is_exact(dev):
    """no decoder: (2^k pred, 2^k target), k = -20, -8, 8, 20, gives the same loss bit for bit and exactly 2^-k times the
    gradient (step_tail_cases.scale_property_inputs checks that the data neither under- nor overflows in float32)"""
    from pde_policylearning_amd import functional as F

    def run(pred, tgt):
        x = pred.detach().clone().requires_grad_(True)
        loss = F.lp_loss_rel(x, tgt)
        loss.backward()
        return loss.detach(), x.grad
    bad = T.scale_property_failures(run, dev)
    assert not bad, "\n".join(bad)


# ---------------------------------------------------------------------------------------------------------------------
# Adam
# ---------------------------------------------------------------------------------------------------------------------
def _adam_engine_bucket(case, p0, grad_of, steps=T.ADAM_CHECK_STEPS, capturable=False, preset=None):
    """FusedAdam on a FlatGradBucket of one parameter; preset: (device step count, exp_avg, exp_avg_sq) to start from"""
    from pde_policylearning_amd.trainer import FlatGradBucket, FusedAdam
    p = torch.nn.Parameter(p0.clone())
    bucket = FlatGradBucket([p])
    opt = FusedAdam(bucket, lr=T.ADAM_LR, betas=T.ADAM_BETAS, eps=T.ADAM_EPS, weight_decay=case["wd"], capturable=capturable)
    assert p.data.data_ptr() == opt.flat_param.data_ptr() and p.grad.data_ptr() == bucket.flat.data_ptr()
    if preset is not None:
        opt.step_dev.fill_(preset[0])
        opt.exp_avg.copy_(preset[1])
        opt.exp_avg_sq.copy_(preset[2])
    out = {}
    for t in range(1, max(steps) + 1):
        p.grad.copy_(grad_of(t))
        opt.step()
        if t in steps:
            out[t] = {"p": opt.flat_param.clone(), "exp_avg": opt.exp_avg.clone(), "exp_avg_sq": opt.exp_avg_sq.clone()}
    return out


def _adam_engine_slots(case, p0, grad_of, steps=T.ADAM_CHECK_STEPS):
    """F.adam_step once per instance and step, each instance in its own slot; the slots' padding must stay as it was"""
    from pde_policylearning_amd import functional as F
    K, n = p0.shape
    pad = 7.25
    bufs = [torch.full((K, T.ADAM_SLOT), pad, device=p0.device) for _ in range(4)]
    P, G, M, V = bufs
    P[:, :n] = p0
    M[:, :n] = 0.0
    V[:, :n] = 0.0
    flat = [b.view(-1) for b in bufs]
    out = {}
    for t in range(1, max(steps) + 1):
        G[:, :n] = grad_of(t)
        for i in range(K):
            lo = i * T.ADAM_SLOT
            F.adam_step(*(f[lo:lo + n] for f in flat), t, lr=T.ADAM_LR, betas=T.ADAM_BETAS, eps=T.ADAM_EPS, weight_decay=case["wd"])
        if t in steps:
            out[t] = {"p": P[:, :n].clone(), "exp_avg": M[:, :n].clone(), "exp_avg_sq": V[:, :n].clone()}
    for b in bufs:
        assert bool((b[:, n:] == pad).all()), "an update wrote past its n elements"
    return out


@pytest.mark.parametrize("case", ADAM_CASES, ids=_ids(ADAM_CASES))
def test_adam_vs_float64(dev, case):
    """p, exp_avg and exp_avg_sq after step 1 and after step 20 against torch.optim.Adam in float64; no floor"""
    case = T.adam_resolve(case, _n_cu(dev))
    p0, grad_of = T.adam_inputs(case, dev)
    got = (_adam_engine_slots if case["n"] <= 5 else _adam_engine_bucket)(case, p0, grad_of)
    ref32, ref64 = T.adam_torch(case, p0, grad_of, torch.float32), T.adam_torch(case, p0, grad_of, torch.float64)
    bad = T.adam_failures(case, got, ref32, ref64)
    assert not bad, "\n".join(bad)


def test_adam_device_counter_equals_host_count_for_50_steps(dev):
    """k_adam_prep (pow in double on the device) against fno_adam_scalars (the host's): p, exp_avg, exp_avg_sq bit for bit
    after every one of 50 steps"""
    case = dict(n=4099, pscale=1e-3, gscale=1.0, wd=1e-4)
    p0, grad_of = T.adam_inputs(case, dev)
    every = tuple(range(1, 51))
    host = _adam_engine_bucket(case, p0, grad_of, steps=every)
    device = _adam_engine_bucket(case, p0, grad_of, steps=every, capturable=True)
    for t in every:
        for k in host[t]:
            assert T.same_bits(host[t][k], device[t][k]), (t, k)


def test_adam_device_counter_preset_to_10000(dev):
    """three steps from a device counter of 10 000 (bias corrections of steps 10 001 .. 10 003, moments given) against
    float64 torch.optim.Adam started from the same state"""
    case = dict(name="adam n=4099 from step 10000", n=4099, pscale=1e-3, gscale=1.0, wd=1e-4)
    p0, grad_of = T.adam_inputs(case, dev)
    g = torch.Generator(device=dev).manual_seed(12)
    m0 = 0.3 * torch.randn(p0.shape, generator=g, device=dev)
    v0 = torch.randn(p0.shape, generator=g, device=dev) ** 2 + 0.01
    steps = (1, 2, 3)
    got = _adam_engine_bucket(case, p0, grad_of, steps=steps, capturable=True, preset=(10000, m0, v0))
    ref32 = T.adam_torch(case, p0, grad_of, torch.float32, steps=steps, state=(10000, m0, v0))
    ref64 = T.adam_torch(case, p0, grad_of, torch.float64, steps=steps, state=(10000, m0, v0))
    bad = T.adam_failures(case, got, ref32, ref64)
    assert not bad, "\n".join(bad)


def test_adam_live_rows_beyond_one_sweep(dev):
    """adam_step_runs on a row-sliced block of more complex pairs than one sweep of k_adam_live's grid, followed by a dense
    run: the live columns and the dense tail against float64 torch.optim.Adam, the dead columns untouched bit for bit"""
    from pde_policylearning_amd import functional as F
    row_len, live = 24, 16
    rows = 8 * _n_cu(dev) * 256 // (live // 2) + 4465          # one sweep of pairs and a ragged second trip
    nd = 1027                                                  # the dense run behind the block
    nb = rows * row_len
    case = dict(name=f"adam_live rows={rows} {live}/{row_len} + dense {nd}", n=nb + nd, pscale=1.0, gscale=1.0, wd=1e-4)
    p0, grad_full = T.adam_inputs(case, dev)
    live_mask = torch.zeros(rows, row_len, dtype=torch.bool, device=dev)
    live_mask[:, :live] = True
    keep = torch.cat([live_mask.view(-1), torch.ones(nd, dtype=torch.bool, device=dev)])

    def grad_of(t):                                            # exactly zero in the dead columns, as the engine leaves it
        return grad_full(t) * keep
    runs = [("rows", 0, rows, row_len, live, 0), ("dense", nb, nd, rows * live)]
    p, m, v = p0.clone(), torch.zeros(rows * live + nd, device=dev), torch.zeros(rows * live + nd, device=dev)
    steps, got = (1, 5), {}
    for t in range(1, 6):
        F.adam_step_runs(runs, p, grad_of(t).contiguous(), m, v, t, T.ADAM_LR, T.ADAM_BETAS, T.ADAM_EPS, case["wd"])
        if t in steps:
            got[t] = {"p": p[keep].clone(), "exp_avg": m.clone(), "exp_avg_sq": v.clone()}
        assert T.same_bits(p[~keep], p0[~keep]), t
    pk = p0[keep]
    ref32 = T.adam_torch(case, pk, lambda t: grad_of(t)[keep], torch.float32, steps=steps)
    ref64 = T.adam_torch(case, pk, lambda t: grad_of(t)[keep], torch.float64, steps=steps)
    bad = T.adam_failures(case, got, ref32, ref64)
    assert not bad, "\n".join(bad)
