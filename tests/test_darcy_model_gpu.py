"""pino_models.FNO2d on an odd grid (its mixed route), train_2d_operator in both loader forms, eval_darcy and eval_burgers on
the GPU against float64 on the CPU.  Cases, the restated loops and the criterion: tests/darcy_cases.py and
tests/burgers_cases.py (the restated model).  Every case asserts its route before any number is compared; every measured
distance goes to profiles/r21_darcy_errors.txt first."""
import os

import numpy as np
import pytest
import torch

from tests import burgers_cases as KB
from tests import darcy_cases as K
from tests.judging import dev, judge_budget  # noqa: F401

pytestmark = pytest.mark.gpu

GLUE = ("k_lift", "k_proj", "k_pw")          # profile labels of the engine's lifting / pointwise kernels
LOSSES = ("k_darcy", "k_burgers", "k_lploss")


def build(dev, p, modes2=K.MODES, **kw):  # noqa: F811
    from pde_policylearning_amd.libs.models.pino_models import FNO2d
    model = FNO2d(modes1=list(K.MODES), modes2=list(modes2), fc_dim=128, layers=[32] * 4, in_dim=3, act="gelu", **kw)
    model.load_state_dict(p)
    return model.to(dev)


def assert_mixed(records, what):
    names = [r["name"] for r in records]
    spectral = [n for n in names if not n.startswith(LOSSES + GLUE)]
    assert spectral, f"{what}: the spectral convolutions run on the engine: {sorted(set(names))}"
    assert not [n for n in names if n.startswith(GLUE)], f"{what}: no lifting / pointwise kernel on an odd grid"


@pytest.mark.parametrize("case", list(K.MODEL_PADS))
def test_fno2d_on_an_odd_grid(dev, case):  # noqa: F811
    """(2, 37, 37, 3), unpadded and padded to 40 x 40: spectral convolutions on the engine, pointwise parts as torch modules"""
    from pde_policylearning_amd import _lib
    pad = K.MODEL_PADS[case]
    p, x = K.model_params("fno2d"), K.model_input()
    model = build(dev, p, pad_ratio=pad)
    with _lib.launch_log() as log:
        y = model(x.to(dev))
        names = [n for n, _ in model.named_parameters()]
        grads = torch.autograd.grad(y.square().sum(), [q for _, q in model.named_parameters()])
        torch.cuda.synchronize()
    assert model.route(x.to(dev)) == "torch"
    assert_mixed(log.records, case)
    got = {"y": y.detach().cpu(), **{"grad " + n: g.cpu() for n, g in zip(names, grads)}}
    ref64 = KB.model_reference(p, x, K.MODES, K.MODES, pad, "gelu", torch.float64)
    ref32 = KB.model_reference(p, x, K.MODES, K.MODES, pad, "gelu", torch.float32)
    judge_budget(K.LOG, f"pino FNO2d odd grid {case}", KB.model_rows(got, ref64, ref32))


def _dataset(form):
    from pde_policylearning_amd.libs.pino_utils.datasets import DarcyCombo, DarcyFlow
    if form == "combo":
        return DarcyCombo(K.train_arrays(), nx=K.TRAIN_NX, sub=K.TRAIN_SUB, pde_sub=K.TRAIN_PDE_SUB, num=K.TRAIN_N)
    return DarcyFlow(K.train_arrays(), nx=K.TRAIN_NX, sub=K.TRAIN_SUB, num=K.TRAIN_N)


@pytest.mark.parametrize("form", ["combo", "flow"])
def test_train_2d_operator_trajectory(dev, tmp_path, monkeypatch, form):  # noqa: F811
    """three epochs, 8 samples in batches of 4 (S 21, equation grid 41), Adam 1e-3, weights xy 5 / f 1: each epoch's
    (train_loss, f_loss, data_loss) under the budget rule against the float64 run of the same loop, the float32 run of
    that restatement as the yardstick"""
    from torch.utils.data import DataLoader
    from pde_policylearning_amd import _lib
    from pde_policylearning_amd.libs.pino_utils.train_2d import train_2d_operator
    monkeypatch.chdir(tmp_path)                              # the loop writes its checkpoint under the working directory
    ds = _dataset(form)
    assert ds.S == 21 and (form == "flow" or ds.pde_S == 41)
    p = K.model_params("train")
    model = build(dev, p)
    opt = torch.optim.Adam(model.parameters(), lr=K.TRAIN_LR)
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=100)
    with _lib.launch_log() as log:
        hist = train_2d_operator(model, DataLoader(ds, batch_size=K.TRAIN_BATCH), opt, sched, K.TRAIN_CFG, rank=dev, use_tqdm=False)
    names = [r["name"] for r in log.records]
    assert names.count("k_darcy_fwd") == 6 and names.count("k_darcy_bwd") == 6
    assert any(n.startswith("k_lploss") for n in names) == (form == "combo")
    assert_mixed(log.records, form)
    assert os.path.exists("checkpoints/darcy_test/d.pt")
    ref64 = K.restated_training(p, ds, form, torch.float64)
    ref32 = K.restated_training(p, ds, form, torch.float32)
    rows = [(f"epoch {e} {q}", K.scalar_err(hist[e][i], ref64[e][i]), K.scalar_err(ref32[e][i], ref64[e][i]), K.FLOOR)
            for e in range(3) for i, q in enumerate(("train_loss", "f_loss", "data_loss"))]
    judge_budget(K.LOG, f"train_2d_operator {form} 3 epochs", rows)


def test_train_2d_operator_without_the_data_term(dev, tmp_path, monkeypatch):  # noqa: F811
    """xy_loss 0 on the three-tuple form: one forward per step, the data loss reported as zero"""
    from torch.utils.data import DataLoader
    from pde_policylearning_amd import _lib
    from pde_policylearning_amd.libs.pino_utils.train_2d import train_2d_operator
    monkeypatch.chdir(tmp_path)
    model = build(dev, K.model_params("train"))
    opt = torch.optim.Adam(model.parameters(), lr=K.TRAIN_LR)
    cfg = {"train": dict(K.TRAIN_CFG["train"], xy_loss=0.0, epochs=1)}
    with _lib.launch_log() as log:
        hist = train_2d_operator(model, DataLoader(_dataset("combo"), batch_size=K.TRAIN_BATCH), opt,
                                 torch.optim.lr_scheduler.StepLR(opt, step_size=100), cfg, rank=dev, use_tqdm=False)
    names = [r["name"] for r in log.records]
    assert not any(n.startswith("k_lploss") for n in names) and names.count("k_darcy_fwd") == 2
    assert hist[0][2] == 0.0 and hist[0][0] == hist[0][1] > 0.0


def _eval_rows(got, ref64, ref32):
    return [(q, K.scalar_err(got[i], ref64[i]), K.scalar_err(ref32[i], ref64[i]), K.FLOOR)
            for i, q in enumerate(("mean_err", "std_err", "mean_f_err", "std_f_err"))]


def test_eval_darcy(dev, capsys):  # noqa: F811
    from torch.utils.data import DataLoader
    from pde_policylearning_amd import _lib
    from pde_policylearning_amd.libs.pino_utils.eval_2d import eval_darcy
    ds, p = _dataset("flow"), K.model_params("train")
    model = build(dev, p)
    with _lib.launch_log() as log:
        got = eval_darcy(model, DataLoader(ds, batch_size=K.TRAIN_BATCH), None, dev, use_tqdm=False)
    names = [r["name"] for r in log.records]
    assert names.count("k_darcy_fwd") == 2 and "k_darcy_bwd" not in names and not any(n.startswith("k_lploss") for n in names)
    printed = capsys.readouterr().out
    assert f"==Averaged relative L2 error mean: {got[0]}, std error: {got[1]}==" in printed
    assert f"==Averaged equation error mean: {got[2]}, std error: {got[3]}==" in printed
    assert all(q.grad is None for q in model.parameters())
    judge_budget(K.LOG, "eval_darcy", _eval_rows(got, K.restated_eval_darcy(p, ds, torch.float64), K.restated_eval_darcy(p, ds, torch.float32)))


def test_eval_burgers(dev, capsys):  # noqa: F811
    from pde_policylearning_amd import _lib
    from pde_policylearning_amd.libs.pino_utils.eval_2d import eval_burgers
    p = KB.golden_params(np.load(os.path.join(KB.GOLDEN, "pino_fno2d_small.npz")))
    batches = K.burgers_batches()
    model = build(dev, p, modes2=KB.MODES2)
    with _lib.launch_log() as log:
        got = eval_burgers(model, batches, K.BURGERS_VISC, None, dev, use_tqdm=False)
    names = [r["name"] for r in log.records]
    assert names.count("k_burgers_fwd") == 2 and "k_burgers_bwd" not in names and any(n.startswith("k_lploss") for n in names)
    assert "==Averaged equation error mean:" in capsys.readouterr().out
    with torch.no_grad():
        ref64, ref32 = (K.restated_eval_burgers(p, batches, dt) for dt in (torch.float64, torch.float32))
    judge_budget(K.LOG, "eval_burgers", _eval_rows(got, ref64, ref32))
