"""The spectral Sobolev loss (csrc/k_hs_loss.h) on the GPU through libs.utilities3.HsLoss, against the float64 restatement of
tests/hs_loss_cases.py.  Every evaluation first asserts from the launch log that only the new kernels ran - two forward
launches and one backward, one workgroup per (sample, channel pair); every measured distance goes to
profiles/r24_hs_loss_errors.txt before anything is asserted."""
import numpy as np
import pytest
import torch

from tests import hs_loss_cases as K
from tests.judging import dev, judge_budget, rel_err  # noqa: F401
from tests.step_tail_cases import same_bits

pytestmark = pytest.mark.gpu

FWD, BWD = ["k_hs_plane_fwd", "k_hs_finish"], ["k_hs_plane_bwd"]


def build(k, a, group, reduce):
    from pde_policylearning_amd.libs.utilities3 import HsLoss
    return HsLoss(k=k, a=None if a is None else list(a), group=group, size_average=reduce == "mean", reduction=reduce is not None)


def evaluate(x, y, dev, k=1, a=None, group=False, reduce="mean", g=None, backward=True):  # noqa: F811
    """{"value"[, "grad"]} on the CPU of one loss call (+ backward with upstream g, default ones) through the class; the route
    is asserted here"""
    from pde_policylearning_amd import _lib
    fn = build(k, a, group, reduce)
    xg, yg = x.to(dev).requires_grad_(backward), y.to(dev)
    assert xg.is_contiguous() == x.is_contiguous()      # a view arrives on the device as the view it is
    up = None if g is None else torch.as_tensor(g, dtype=torch.float32).to(dev)
    with _lib.launch_log() as log:
        val = fn(xg, yg)
        if backward:
            val.backward(torch.ones_like(val) if up is None else up.reshape(val.shape))
        torch.cuda.synchronize()
    names = [r["name"] for r in log.records]
    assert names == FWD + (BWD if backward else []), names
    n, channels = x.shape[1], int(np.prod(x.shape[3:], dtype=np.int64))
    planes = x.shape[0] * ((channels + 1) // 2)
    assert log.records[0]["grid"] == (planes, 1, 1) and (not backward or log.records[2]["grid"] == (planes, 1, 1))
    assert log.records[0]["block"] == ((1024 if n == 128 else 512), 1, 1) and log.records[1]["grid"] == (1, 1, 1)
    assert val.shape == (() if reduce is not None else (x.shape[0],))
    got = {"value": val.detach().cpu()}
    if backward:
        assert xg.grad.shape == x.shape
        got["grad"] = xg.grad.cpu()
    return got


@pytest.mark.parametrize("shape", K.SHAPES, ids=[K.shape_id(s) for s in K.SHAPES])
def test_loss_vs_float64(dev, shape):  # noqa: F811
    """loss (mean: default upstream gradient; sum: 0.37), per-sample values (a non-uniform (B,) upstream gradient) and dx of
    every form and family"""
    rows = []
    for family in K.FAMILIES:
        for k, a, group in K.FORMS:
            for reduce in K.REDUCTIONS:
                g = K.upstream(reduce, shape[0])
                x, y, ref64, ref32 = K.references(family, shape, k, a, group, reduce, g)
                got = evaluate(x, y, dev, k, a, group, reduce, g)
                rows += K.loss_rows(got, ref64, ref32, K.combo_name(family, k, a, group, reduce))
    judge_budget(K.LOG, "loss " + K.shape_id(shape), rows, width=58)


@pytest.mark.parametrize("n", [32, 128])
def test_single_modes(dev, n):  # noqa: F811
    """x - y and y one cosine mode each: the loss is amplitude ratio x sqrt(W(p, q) / W(p', q')).  A weight evaluated at the
    wrong bit-reversed bin, or a Nyquist row taken as -n/2 without the absolute value (or dropped), moves it by a factor.
    Tolerance 1e-5 (judging.TOL_G): the float32 rounding of x = y + e leaves white noise of 6e-8 |y| in e, which the |k|^4
    weight (a[1]^2 (n^2 / 2)^2 = 4e6 at n = 128) lifts to at most 3e-6 of a mode of weight 1."""
    from tests.judging import TOL_G
    pairs = K.mode_pairs(n)
    k, a = 2, (0.5, 0.25)
    lines, bad = [], []
    for i, pe in enumerate(pairs):
        py = pairs[(i + 1) % len(pairs)]
        y64 = K.cosine_mode(n, *py, 1.0)
        y = torch.from_numpy(y64.astype(np.float32)).reshape(1, n, n)
        x = torch.from_numpy((y.numpy().reshape(n, n).astype(np.float64) + K.cosine_mode(n, *pe, 0.5)).astype(np.float32)).reshape(1, n, n)
        want = K.mode_loss(n, pe, 0.5, py, 1.0, k, a)
        truth = float(K.restated(x, y, torch.float64, k, a)["value"])
        got = float(evaluate(x, y, dev, k, a, backward=False)["value"])
        err, err64 = abs(got - want) / want, abs(truth - want) / want
        lines.append(f"e {pe} y {py}: closed form {want:.9e}   engine {got:.9e} ({err:9.2e})   float64 restatement ({err64:9.2e})   "
                     f"{'ok' if err < TOL_G and err64 < TOL_G else 'MISS'}")
        if not (err < TOL_G and err64 < TOL_G):
            bad.append(lines[-1])
    section = f"single modes n={n}"
    for line in lines:
        print(section, line)
    K.LOG.replace(section, lines)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("shape", [(3, 32, 32), (2, 32, 32, 3), (1, 128, 128, 2)], ids=K.shape_id)
def test_bitwise_repeatable(dev, shape):  # noqa: F811
    x, y = K.make_inputs("white", shape)
    for k, a, group, reduce in ((2, (0.5, 0.25), False, "mean"), (2, (0.5, 0.25), True, None)):
        one, two = evaluate(x, y, dev, k, a, group, reduce), evaluate(x, y, dev, k, a, group, reduce)
        for name in one:
            assert same_bits(one[name].reshape(-1), two[name].reshape(-1)), (k, group, name)


@pytest.mark.parametrize("shape", [(3, 32, 32), (3, 32, 32, 3), (3, 64, 64, 2)], ids=K.shape_id)
def test_a_sample_does_not_depend_on_its_batch(dev, shape):  # noqa: F811
    """sample b of a B = 3 batch under reduction=False and its own B = 1 run: the same bits, value and dx row.  The channels of
    a sample enter through ONE fixed order - the pairs (0, 1), (2, 3), .. are each summed over the bins by their own
    workgroup, and the finishing kernel adds the pairs in ascending order - so permuting channels may change the last bits
    and nothing else."""
    x, y = K.make_inputs("white", shape)
    for k, a, group in ((1, None, False), (2, (0.5, 0.25), True)):
        whole = evaluate(x, y, dev, k, a, group, None)
        for b in range(shape[0]):
            one = evaluate(x[b:b + 1], y[b:b + 1], dev, k, a, group, None)
            assert same_bits(one["value"].reshape(1), whole["value"][b].reshape(1)), (k, group, b)
            assert same_bits(one["grad"][0], whole["grad"][b]), (k, group, b)
    if len(shape) > 3:
        perm = list(range(shape[3]))[::-1]
        base, swapped = evaluate(x, y, dev, reduce=None), evaluate(x[..., perm], y[..., perm], dev, reduce=None)
        assert rel_err(swapped["value"], base["value"]) < 1e-6 and rel_err(swapped["grad"][..., perm], base["grad"]) < 1e-6


def test_equal_fields_give_a_zero_loss_and_a_zero_gradient(dev):  # noqa: F811
    """x == y: loss 0 and dx all zeros, finite (the reference's autograd gives NaN; the stated deviation)"""
    for shape in ((2, 32, 32, 3), (1, 128, 128, 2)):
        _, y = K.make_inputs("white", shape)
        for k, a, group, reduce in ((1, None, False, "mean"), (2, (0.5, 0.25), True, None), (0, None, True, "sum")):
            got = evaluate(y, y, dev, k, a, group, reduce)
            assert not bool(got["value"].any()) and not bool(got["grad"].any()), (shape, k, group)
            assert bool(torch.isfinite(got["grad"]).all())


def test_an_equal_sample_beside_a_live_one(dev):  # noqa: F811
    """one sample with x == y: its row of dx is zero and the other sample is judged as usual"""
    shape = (2, 32, 32, 3)
    x, y = K.make_inputs("white", shape)
    x = x.clone()
    x[0] = y[0]
    rows = []
    for k, a, group in ((1, None, False), (2, (0.5, 0.25), True)):
        for reduce in K.REDUCTIONS:
            g = K.upstream(reduce, 2)
            ref64, ref32 = (K.restated(x, y, t, k, a, group, reduce, g) for t in (torch.float64, torch.float32))
            got = evaluate(x, y, dev, k, a, group, reduce, g)
            assert not bool(got["grad"][0].any()) and bool(got["grad"][1].any())
            rows += K.loss_rows(got, ref64, ref32, K.combo_name("x0==y0", k, a, group, reduce))
    judge_budget(K.LOG, "an equal sample beside a live one " + K.shape_id(shape), rows, width=58)


def test_a_zero_target_is_ieee(dev):  # noqa: F811
    """y = 0 on one sample: inf in the forward, the other sample's value untouched; no backward is taken"""
    shape = (2, 32, 32, 3)
    x, y = K.make_inputs("white", shape)
    y = y.clone()
    y[1] = 0
    for k, a, group in ((1, None, False), (2, (0.5, 0.25), True)):
        got = evaluate(x, y, dev, k, a, group, None, backward=False)["value"]
        ref = K.restated(x, y, torch.float64, k, a, group, None)["samples"]
        assert bool(torch.isinf(got[1])) and got[1] > 0 and abs(float(got[0]) - float(ref[0])) < 1e-5 * float(ref[0])
        assert bool(torch.isinf(evaluate(x, y, dev, k, a, group, "mean", backward=False)["value"]))


def test_non_contiguous_input(dev):  # noqa: F811
    """x as a permuted view of a (B, C, N, N) tensor: the bits of the contiguous copy"""
    shape = (2, 32, 32, 3)
    x, y = K.make_inputs("white", shape)
    view = x.permute(0, 3, 1, 2).contiguous().permute(0, 2, 3, 1)
    assert not view.is_contiguous() and not view.to(dev).is_contiguous() and torch.equal(view, x)
    for k, a, group, reduce in ((1, None, False, "mean"), (2, (0.5, 0.25), True, None)):
        base, got = evaluate(x, y, dev, k, a, group, reduce), evaluate(view, y, dev, k, a, group, reduce)
        assert same_bits(got["value"].reshape(-1), base["value"].reshape(-1)) and same_bits(got["grad"], base["grad"])


def test_refusals_on_the_gpu(dev):  # noqa: F811
    from pde_policylearning_amd import functional as F
    from pde_policylearning_amd.libs.utilities3 import HsLoss
    x = torch.zeros(2, 32, 32, 3, device=dev)
    assert F.hs_loss_supported(x) and not F.hs_loss_supported(x.double()) and not F.hs_loss_supported(x[:, :, :16])
    with pytest.raises(RuntimeError, match="`x` must be float32"):
        HsLoss()(x.double(), x.double())
    with pytest.raises(RuntimeError, match="`y` must be torch.float32"):
        HsLoss()(x, x.double())
    with pytest.raises(RuntimeError, match="`y` must have shape"):
        HsLoss()(x, x[:1])
    with pytest.raises(RuntimeError, match="`y` must live on"):
        HsLoss()(x, x.cpu())
    with pytest.raises(RuntimeError, match="32, 64, 128"):
        HsLoss()(x[:, :, :16], x[:, :, :16])


def test_train_step(dev):  # noqa: F811
    """HsLoss(k=1) as the loss_fn of trainer.train_step on a small FNO2d: the returned loss is HsLoss applied to the model's
    output directly (and the restated float64 loss of that output), and a GraphedTrainStep replay equals the eager step bit
    for bit, loss and parameters (zero learning rate: the same step)"""
    from oracle.detfill import fill_named
    from pde_policylearning_amd.libs.utilities3 import HsLoss
    from pde_policylearning_amd.neuralop.models import FNO2d
    from pde_policylearning_amd.trainer import FlatGradBucket, FusedAdam, GraphedTrainStep, train_step
    torch.manual_seed(0)
    model = FNO2d(8, 8, 32).to(dev)
    x = torch.from_numpy(fill_named("hs.step.x", (2, 3, 32, 32), 1.0)).to(dev)
    tgt = torch.from_numpy(fill_named("hs.step.t", (2, 32, 32, 1), 1.0)).to(dev)
    model_fn = lambda inp: model(inp).permute(0, 2, 3, 1)      # noqa: E731  (channels last, as HsLoss reads its operands)
    loss_fn = HsLoss(k=1)
    bucket = FlatGradBucket(model.parameters(), direct_module=model)
    opt = FusedAdam(bucket, lr=0.0, weight_decay=0.0, capturable=True)
    with torch.no_grad():
        pred = model_fn(x)
        direct = loss_fn(pred, tgt)
    loss = train_step(model_fn, bucket, opt, (x,), tgt, loss_fn)
    eager = (loss.clone(), bucket.flat.clone())
    assert loss.dim() == 0 and bool(bucket.flat.any())
    assert same_bits(loss.reshape(1), direct.reshape(1))
    ref64, ref32 = (K.restated(pred.cpu(), tgt.cpu(), t) for t in (torch.float64, torch.float32))
    judge_budget(K.LOG, "train_step FNO2d(8, 8, 32) (2, 3, 32, 32)", K.loss_rows({"value": loss.cpu()}, ref64, ref32))
    step = GraphedTrainStep(model_fn, bucket, opt, (x,), tgt, loss_fn)
    for rep in range(2):
        replay = step()
        assert same_bits(replay.reshape(1), eager[0].reshape(1)) and same_bits(bucket.flat, eager[1]), rep
