"""pino_models.FNO2d and train_2d_burger on the GPU against float64 on the CPU: the two golden models (the reference's own
float32 output and gradients are the yardstick), the mixed routes, three epochs of the training loop and two steps through a
direct-write gradient bucket.  Cases, the restated model and the criterion: tests/burgers_cases.py.  Every case asserts its
route before any number is compared; every measured distance goes to profiles/r20_burgers_errors.txt first."""
import os

import numpy as np
import pytest
import torch

from tests import burgers_cases as K
from tests.judging import BUDGET_SLACK, dev, judge_budget, rel_err  # noqa: F401

pytestmark = pytest.mark.gpu

GM = np.load(os.path.join(K.GOLDEN, "pino_fno2d_small.npz"))
GLUE = ("k_lift", "k_proj", "k_pw")          # profile labels of the engine's lifting / pointwise kernels


def build(dev, p, **kw):  # noqa: F811
    from pde_policylearning_amd.libs.models.pino_models import FNO2d
    args = dict(modes1=list(K.MODES1), modes2=list(K.MODES2), fc_dim=128, layers=[32] * 4, in_dim=3, act="gelu")
    args.update(kw)
    model = FNO2d(**args)
    if p is not None:
        model.load_state_dict(p)
    return model.to(dev)


def evaluate(model, x, dev):  # noqa: F811
    """({"y", "grad <name>"} on the CPU, launch records, calls of the torch Conv1d modules, calls of the activation)"""
    from pde_policylearning_amd import _lib
    calls = {"conv": 0, "act": 0}
    hooks = [w.register_forward_hook(lambda *a: calls.__setitem__("conv", calls["conv"] + 1)) for w in model.ws]
    act = model.act

    def counted(t):
        calls["act"] += 1
        return act(t)
    model.act = counted
    try:
        with _lib.launch_log() as log:
            y = model(x.to(dev))
            names = [n for n, _ in model.named_parameters()]
            grads = torch.autograd.grad(y.square().sum(), [q for _, q in model.named_parameters()])
            torch.cuda.synchronize()
    finally:
        model.act = act
        for h in hooks:
            h.remove()
    return {"y": y.detach().cpu(), **{"grad " + n: g.cpu() for n, g in zip(names, grads)}}, log.records, calls


def assert_route(records, calls, engine, layers=3):
    """engine: lifting and one pointwise kernel pair per layer on the engine, no torch Conv1d, the activation in the head
    only; otherwise the spectral convolutions alone are engine launches"""
    glue = [r["name"] for r in records if r["name"].startswith(GLUE)]
    assert records, "the spectral convolutions run on the engine on every route"
    if engine:
        assert glue and calls == {"conv": 0, "act": 2}, (glue, calls)
    else:
        assert not glue and calls == {"conv": layers, "act": layers - 1 + 2}, (glue, calls)


@pytest.mark.parametrize("case", list(K.MODEL_CASES))
def test_golden_models(dev, case):  # noqa: F811
    pad = K.MODEL_CASES[case]["pad_ratio"]
    p, x = K.golden_params(GM), K.model_input("pino_fno2d_small")
    model = build(dev, p, pad_ratio=pad)
    got, records, calls = evaluate(model, x, dev)
    assert_route(records, calls, engine=model.route(x.to(dev)) == "chain")
    if case == "pad0":
        assert model.route(x.to(dev)) == "chain", "the unpadded (12, 32) grid is covered by the lifting and layer kernels"
    ref64 = K.model_reference(p, x, K.MODES1, K.MODES2, pad, "gelu", torch.float64)
    own32 = K.model_reference(p, x, K.MODES1, K.MODES2, pad, "gelu", torch.float32)
    # the yardstick is the reference's own float32 run; its spectral gradients are stored for the first GOLDEN_CIN input
    # channels and judged there, and the whole tensors against the float32 run of the restated model
    gold, got_g, ref_g = {"y": torch.from_numpy(GM[f"{case}/y"])}, {"y": got["y"]}, {"y": ref64["y"]}
    for k in ref64:
        if k == "y":
            continue
        g = torch.from_numpy(GM[f"{case}/grads/{k[5:]}"])
        if "sp_convs" in k:
            gold[k + f" [:{K.GOLDEN_CIN}]"] = torch.view_as_complex(g)
            got_g[k + f" [:{K.GOLDEN_CIN}]"], ref_g[k + f" [:{K.GOLDEN_CIN}]"] = got[k][:K.GOLDEN_CIN], ref64[k][:K.GOLDEN_CIN]
            gold[k], got_g[k], ref_g[k] = own32[k], got[k], ref64[k]
        else:
            gold[k], got_g[k], ref_g[k] = g, got[k], ref64[k]
    judge_budget(K.LOG, f"pino FNO2d golden {case}", K.model_rows(got_g, ref_g, gold))


@pytest.mark.parametrize("variant", ["relu", "widths"])
def test_mixed_routes(dev, variant):  # noqa: F811
    """act='relu' and layers=[32, 32, 64, 64]: spectral convolutions on the engine, pointwise parts as torch modules"""
    kw = {"relu": dict(act="relu"), "widths": dict(layers=[32, 32, 64, 64])}[variant]
    model = build(dev, None, **kw)
    p = {}
    for n, v in model.state_dict().items():
        scale = 1.0 / v.shape[0] if v.is_complex() else (0.1 if v.dim() == 1 else 1.0 / v.shape[1] ** 0.5)
        p[n] = torch.from_numpy(np.asarray(K.fill_named(f"fno2d.{variant}.{n}", tuple(v.shape), scale, complex_=v.is_complex())))
    model.load_state_dict(p)
    x = K.model_input("fno2d." + variant)
    got, records, calls = evaluate(model, x, dev)
    assert model.route(x.to(dev)) == "torch"
    assert_route(records, calls, engine=False)
    act = kw.get("act", "gelu")
    ref64 = K.model_reference(p, x, K.MODES1, K.MODES2, [0., 0.], act, torch.float64)
    ref32 = K.model_reference(p, x, K.MODES1, K.MODES2, [0., 0.], act, torch.float32)
    judge_budget(K.LOG, f"pino FNO2d mixed {variant}", K.model_rows(got, ref64, ref32))


def test_train_2d_burger_trajectory(dev, tmp_path, monkeypatch):  # noqa: F811
    """three epochs, one batch of 2, Adam 1e-3, weights xy 1 / f 1 / ic 5: each epoch's (train_loss, train_pino, data_l2)
    within max(2e-6, 1.75 x the reference's float32 trajectory's own distance) of the float64 run of the same loop"""
    from pde_policylearning_amd import _lib
    from pde_policylearning_amd.libs.pino_utils.train_2d import train_2d_burger
    monkeypatch.chdir(tmp_path)                              # the loop writes checkpoints under the working directory
    p = K.golden_params(GM)
    x, y = K.train_data()
    model = build(dev, p)
    opt = torch.optim.Adam(model.parameters(), lr=K.TRAIN_LR)
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=100)
    with _lib.launch_log() as log:
        hist = train_2d_burger(model, [(x, y)], K.TRAIN_VISC, opt, sched, K.TRAIN_CFG, rank=dev, use_tqdm=False)
    names = [r["name"] for r in log.records]
    assert names.count("k_burgers_fwd") == 3 and names.count("k_burgers_bwd") == 3 and any(n.startswith("k_lploss") for n in names)
    assert os.path.exists("checkpoints/burgers_test/t_0.pt") and os.path.exists("checkpoints/burgers_test/t.pt")
    ref64 = K.restated_training(p, x, y, K.MODES1, K.MODES2, [0., 0.], torch.float64)
    gold = GM["train/history"]
    rows = []
    for e in range(3):
        for i, q in enumerate(("train_loss", "train_pino", "data_l2")):
            rows.append((f"epoch {e} {q}", K.scalar_err(hist[e][i], ref64[e][i]), K.scalar_err(gold[e][i], ref64[e][i]), K.FLOOR))
    judge_budget(K.LOG, "train_2d_burger 3 epochs", rows)


def test_second_step_through_a_direct_write_bucket_is_a_fresh_gradient(dev):  # noqa: F811
    """trainer.FlatGradBucket(direct_module=model) marks the spectral convolutions' engine-written gradients and never clears
    them: after two steps on different data every p.grad is the SECOND step's gradient (1e-6 relative L2 against a fresh
    evaluation of step 2 without a bucket, as tests/test_fno1d_gpu.py holds FNO1d)"""
    from pde_policylearning_amd.trainer import FlatGradBucket
    p = K.golden_params(GM)
    models = [build(dev, p), build(dev, p)]
    data = [K.model_input(f"fno2d.bucket{i}").to(dev) for i in (1, 2)]
    bucket = FlatGradBucket(models[0].parameters(), direct_module=models[0])
    for x in data:
        bucket.zero()
        models[0](x).square().sum().backward()
    names = [n for n, _ in models[1].named_parameters()]
    fresh = torch.autograd.grad(models[1](data[1]).square().sum(), [q for _, q in models[1].named_parameters()])
    got = dict(models[0].named_parameters())
    re = lambda t: torch.view_as_real(t.resolve_conj()) if t.is_complex() else t      # noqa: E731
    errs = {n: rel_err(re(got[n].grad).cpu(), re(f).cpu()) for n, f in zip(names, fresh)}
    K.LOG.replace("bucket second step FNO2d", [f"{n:40s} step-2 gradient vs fresh {e:.3e}   bound 1.0e-06" for n, e in errs.items()])
    assert max(errs.values()) <= 1e-6, errs
