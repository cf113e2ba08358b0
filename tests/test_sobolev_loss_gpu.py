"""The Sobolev / L2 training losses (csrc/k_sobolev_loss.h) on the GPU through neuralop.training.losses LpLoss / H1Loss,
against the float64 restatement of tests/sobolev_cases.py.  Every evaluation first asserts from the launch log that only the
new kernels ran - two forward launches and one backward; every measured distance goes to
profiles/r23_sobolev_loss_errors.txt before anything is asserted."""
import math

import pytest
import torch

from tests import sobolev_cases as K
from tests.judging import dev, judge_budget  # noqa: F401
from tests.step_tail_cases import same_bits

pytestmark = pytest.mark.gpu

FWD, BWD = ["k_sobolev_fwd", "k_sobolev_finish"], ["k_sobolev_bwd"]


def tiles(shape, d, order):
    grid = shape[len(shape) - d:]
    if not order:
        return -(-math.prod(grid) // K.T0)
    t = {1: (K.T1,), 2: K.T2, 3: K.T3}[d]
    return math.prod(-(-n // tk) for n, tk in zip(grid, t))


def build(d, order, fix, reduce_dims, reductions, L):
    from pde_policylearning_amd.neuralop.training import H1Loss, LpLoss
    if order:
        flags = dict(zip(("fix_x_bnd", "fix_y_bnd", "fix_z_bnd"), fix))
        return H1Loss(d=d, L=L, reduce_dims=reduce_dims, reductions=reductions, **flags)
    return LpLoss(d=d, L=L, reduce_dims=reduce_dims, reductions=reductions)


def evaluate(x, y, d, dev, order=1, relative=True, fix=None, reduce_dims=0, reductions="sum", L=K.L_DEFAULT, h=None, g=None,  # noqa: F811
             backward=True):
    """{"value"[, "grad"]} on the CPU of one loss call (+ backward with upstream g, default ones) through the classes; the
    route is asserted here"""
    from pde_policylearning_amd import _lib
    fn = build(d, order, (False,) * d if fix is None else fix, reduce_dims, reductions, L)
    xg, yg = x.to(dev).requires_grad_(backward), y.to(dev)
    up = None if g is None else torch.as_tensor(g, dtype=torch.float32).to(dev)
    with _lib.launch_log() as log:
        if relative:
            val = fn.rel(xg, yg, h=h) if order else fn.rel(xg, yg)
        else:
            val = fn.abs(xg, yg, h=h)
        if backward:
            val.backward(torch.ones_like(val) if up is None else up.reshape(val.shape))
        torch.cuda.synchronize()
    lead = x.shape[:x.dim() - d]
    names = [r["name"] for r in log.records]
    assert names == FWD + (BWD if backward else []), names
    n = math.prod(lead) * tiles(tuple(x.shape), d, order)
    assert log.records[0]["grid"] == (n, 1, 1) and (not backward or log.records[2]["grid"] == (n, 1, 1))
    assert all(r["block"] == (256, 1, 1) for r in log.records)
    got = {"value": val.detach().cpu()}
    if backward:
        got["grad"] = xg.grad.cpu()
    return got


@pytest.mark.parametrize("shape,d", K.SHAPES, ids=[K.shape_id(s, d) for s, d in K.SHAPES])
def test_loss_vs_float64(dev, shape, d):  # noqa: F811
    """values and dx of every family, H1 in every boundary mode (mixed per-axis flags included) and Lp, rel and abs, with the
    default reduction (sum over the batch inside the engine)"""
    rows = []
    for family in K.FAMILIES:
        for order, rel, fix in K.combos(d):
            x, y, h, ref64, ref32 = K.references(family, shape, d, order, rel, fix)
            got = evaluate(x, y, d, dev, order, rel, fix)
            assert got["value"].shape == ref64["value"].shape
            rows += K.loss_rows(got, ref64, ref32, d, K.combo_name(family, order, rel, fix))
    judge_budget(K.LOG, "loss " + K.shape_id(shape, d), rows, width=40)


@pytest.mark.parametrize("shape,d", [((3, 2, 17, 33), 2), ((2, 2, 5), 1), ((2, 2, 5, 6, 7), 3)])
def test_mesh_widths(dev, shape, d):  # noqa: F811
    """a list L, an explicit list h and an explicit float h, fixed and periodic"""
    rows = []
    Ls = tuple(1.0 + 0.5 * k for k in range(d))
    hs = tuple(0.3 + 0.2 * k for k in range(d))
    for name, kw in (("L list", dict(L=Ls)), ("h list", dict(h=hs)), ("h float", dict(h=0.25))):
        for order, rel, fix in ((1, True, (True,) * d), (1, False, (False,) * d), (0, False, (False,) * d)):
            x, y, h, ref64, ref32 = K.references("white", shape, d, order, rel, fix, **kw)
            args = {k: (list(v) if isinstance(v, tuple) else v) for k, v in kw.items()}
            got = evaluate(x, y, d, dev, order, rel, fix, **args)
            rows += K.loss_rows(got, ref64, ref32, d, f"{name:8s}" + K.combo_name("white", order, rel, fix))
    judge_budget(K.LOG, "mesh widths " + K.shape_id(shape, d), rows, width=48)


@pytest.mark.parametrize("reduce_dims,reductions", [((0,), ("sum",)), ((0,), ("mean",)), (None, ("sum",)), ((0, 1), ("sum", "mean")),
                                                    ((0, 1), ("mean", "sum")), ((1,), ("mean",))])
def test_reductions_and_upstream_gradients(dev, reduce_dims, reductions):  # noqa: F811
    """the fused batch reduction (sum, mean), the per-plane tensor and reduce_dims the engine does not fuse, each with a
    non-unit upstream gradient of the result's shape (per channel, per plane, scalar); output shapes are the reference's"""
    shape, d = (2, 3, 61, 61), 2
    want = {(0,): (3,), None: (2, 3), (0, 1): (), (1,): (2,)}[reduce_dims]
    g = (torch.arange(math.prod(want), dtype=torch.float64).reshape(want) * 0.9 - 1.3).tolist()
    rows = []
    for order, rel, fix in ((1, True, (True, False)), (1, False, (False, False)), (0, True, (False, False))):
        x, y = K.make_inputs("smooth", shape, d)
        h = K.uniform_h(shape, d)
        kw = dict(order=order, relative=rel, fix=fix, reduce_dims=reduce_dims, reductions=reductions, g=g)
        ref64, ref32 = K.restated(x, y, d, h, torch.float64, **kw), K.restated(x, y, d, h, torch.float32, **kw)
        got = evaluate(x, y, d, dev, order, rel, fix, None if reduce_dims is None else list(reduce_dims), list(reductions), g=g)
        assert got["value"].shape == want
        rows += K.loss_rows(got, ref64, ref32, d, K.combo_name("smooth", order, rel, fix))
    judge_budget(K.LOG, f"reductions {reduce_dims} {reductions}", rows, width=40)


def test_output_shapes(dev):  # noqa: F811
    """(B, C, grid) gives (C,), C = 1 a 0-d tensor, a (B, n) input with no channel axis a 0-d tensor, reduce_dims=None `lead`"""
    for shape, d, reduce_dims, want in (((2, 3, 5, 4), 2, 0, (3,)), ((2, 1, 5, 4), 2, 0, ()), ((4, 9), 1, 0, ()), ((2, 3, 5, 4), 2, None, (2, 3)),
                                        ((5, 4), 2, None, ()), ((2, 1, 3, 5, 4), 3, 0, ()), ((2, 2, 3, 5, 4), 2, 0, (2, 3))):
        x, y = K.make_inputs("white", shape, d)
        for order in (1, 0):
            got = evaluate(x, y, d, dev, order, reduce_dims=reduce_dims)
            assert got["value"].shape == want and got["grad"].shape == x.shape, (shape, reduce_dims, got["value"].shape)
            ref = K.restated(x, y, d, K.uniform_h(shape, d), torch.float64, order=order, reduce_dims=None if reduce_dims is None else (0,))
            assert K.rel_err(got["value"], ref["value"].reshape(want)) < 1e-5 and K.rel_err(got["grad"], ref["grad"]) < 1e-5


@pytest.mark.parametrize("shape,d", [((2, 3, 61, 61), 2), ((2, 1, 2 * K.T1 + 1), 1), ((2, 2, 5, 6, 7), 3), ((1, 1, 65 * K.T1 + 3), 1)])
def test_bitwise_repeatable(dev, shape, d):  # noqa: F811
    x, y = K.make_inputs("white", shape, d)
    for order, fix in ((1, (True,) * d), (0, None)):
        a, b = evaluate(x, y, d, dev, order, fix=fix), evaluate(x, y, d, dev, order, fix=fix)
        for k in a:
            assert same_bits(a[k].reshape(-1), b[k].reshape(-1)), (order, k)


@pytest.mark.parametrize("shape,d", [((2, 3, 61, 61), 2), ((3, 2, 2 * K.T1 + 1), 1), ((2, 2, 5, 6, 7), 3)])
def test_a_plane_does_not_depend_on_its_batch(dev, shape, d):  # noqa: F811
    """a plane's value and gradient computed alone and inside the larger call: the same bits"""
    x, y = K.make_inputs("white", shape, d)
    for order, rel, fix in ((1, True, (True,) * d), (1, False, None), (0, True, None)):
        whole = evaluate(x, y, d, dev, order, rel, fix, reduce_dims=None)
        for b, c in ((0, 0), (shape[0] - 1, shape[1] - 1)):
            one = evaluate(x[b:b + 1, c:c + 1], y[b:b + 1, c:c + 1], d, dev, order, rel, fix, reduce_dims=None)
            assert same_bits(one["value"].reshape(1), whole["value"][b, c].reshape(1)), (order, b, c)
            assert same_bits(one["grad"][0, 0], whole["grad"][b, c]), (order, b, c)


def test_input_forms(dev):  # noqa: F811
    """a non-contiguous x (copied) gives the bits of the contiguous one; a (B, n) input has no channel axis"""
    shape, d = (2, 3, 61, 61), 2
    x, y = K.make_inputs("white", shape, d)
    base = evaluate(x, y, d, dev, fix=(True, True))
    strided = x.transpose(2, 3).contiguous().transpose(2, 3)
    assert not strided.is_contiguous() and torch.equal(strided, x)
    got = evaluate(strided, y, d, dev, fix=(True, True))
    assert same_bits(got["value"], base["value"]) and same_bits(got["grad"], base["grad"])
    x1, y1 = K.make_inputs("smooth", (4, 1025), 1)
    rows = []
    for order in (1, 0):
        ref64, ref32 = (K.restated(x1, y1, 1, K.uniform_h((4, 1025), 1), t, order=order) for t in (torch.float64, torch.float32))
        rows += K.loss_rows(evaluate(x1, y1, 1, dev, order), ref64, ref32, 1, f"order {order} ")
    judge_budget(K.LOG, "input forms (4, 1025)", rows)


def test_refusals_on_the_gpu(dev):  # noqa: F811
    from pde_policylearning_amd import functional as F
    from pde_policylearning_amd.neuralop.training import H1Loss
    x = torch.zeros(2, 3, 8, 8, device=dev)
    assert F.sobolev_loss_supported(x, 2) and not F.sobolev_loss_supported(x.double(), 2) and not F.sobolev_loss_supported(x[..., :1], 2)
    with pytest.raises(RuntimeError, match="`x` must be float32"):
        H1Loss(d=2)(x.double(), x.double())
    with pytest.raises(RuntimeError, match="`y` must be torch.float32"):
        H1Loss(d=2)(x, x.double())
    with pytest.raises(RuntimeError, match="`y` must have shape"):
        H1Loss(d=2)(x, x[:1])
    with pytest.raises(RuntimeError, match="`y` must live on"):
        H1Loss(d=2)(x, x.cpu())
    with pytest.raises(RuntimeError, match="`y` must be data"):
        H1Loss(d=2)(x, x.clone().requires_grad_(True))
    with pytest.raises(RuntimeError, match="extent 1"):
        H1Loss(d=2)(x[..., :1], x[..., :1])


def test_equal_fields_give_a_zero_loss_and_a_zero_gradient(dev):  # noqa: F811
    """x == y: the reference's autograd gives NaN; the engine's stated deviation is zeros"""
    for shape, d in (((2, 3, 61, 61), 2), ((2, 2, 5), 1), ((2, 2, 5, 6, 7), 3)):
        _, y = K.make_inputs("white", shape, d)
        for order, rel in ((1, True), (1, False), (0, True), (0, False)):
            got = evaluate(y, y, d, dev, order, rel, (True,) * d)
            assert not bool(got["value"].any()) and not bool(got["grad"].any()), (shape, order, rel)


def test_train_step(dev):  # noqa: F811
    """H1Loss(d=2) as the loss_fn of trainer.train_step on a small FNO2d: the loss is the restated float64 loss of the
    model's own output, and a GraphedTrainStep replay equals the eager step bit for bit (zero learning rate: the same step)"""
    from oracle.detfill import fill_named
    from pde_policylearning_amd.neuralop.models import FNO2d
    from pde_policylearning_amd.neuralop.training import H1Loss
    from pde_policylearning_amd.trainer import FlatGradBucket, FusedAdam, GraphedTrainStep, train_step
    torch.manual_seed(0)
    model = FNO2d(8, 8, 32).to(dev)
    x = torch.from_numpy(fill_named("sobolev.step.x", (2, 3, 32, 32), 1.0)).to(dev)
    tgt = torch.from_numpy(fill_named("sobolev.step.t", (2, 1, 32, 32), 1.0)).to(dev)
    loss_fn = H1Loss(d=2)
    bucket = FlatGradBucket(model.parameters(), direct_module=model)
    opt = FusedAdam(bucket, lr=0.0, weight_decay=0.0, capturable=True)
    with torch.no_grad():
        pred = model(x).cpu()
    loss = train_step(model, bucket, opt, (x,), tgt, loss_fn)
    eager = (loss.clone(), bucket.flat.clone())
    assert loss.dim() == 0 and bool(bucket.flat.any())
    h = K.uniform_h((2, 1, 32, 32), 2)
    ref64, ref32 = (K.restated(pred, tgt.cpu(), 2, h, t) for t in (torch.float64, torch.float32))
    judge_budget(K.LOG, "train_step FNO2d(8, 8, 32) (2, 3, 32, 32)", K.loss_rows({"value": loss.cpu()}, ref64, ref32, 2))
    step = GraphedTrainStep(model, bucket, opt, (x,), tgt, loss_fn)
    for rep in range(2):
        replay = step()
        assert same_bits(replay.reshape(1), eager[0].reshape(1)) and same_bits(bucket.flat, eager[1]), rep
