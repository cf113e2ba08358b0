"""Generate tests/golden/burgers_loss_small.npz and pino_fno2d_small.npz from the reference, on the CPU in float32.

    python tools/make_burgers_golden.py --ref DIR        # DIR: a checkout of the reference project

burgers_loss_small.npz: the reference's own PINO_loss / FDM_Burgers (libs/pino_utils/losses.py:200-243) on the inputs of
tests/burgers_cases.py::GOLDEN_CASES with visc 0.01: loss_u, loss_f, the residual field and autograd's du of
5 loss_u + loss_f, under "<family>_<B>_<nt>_<nx>/".
pino_fno2d_small.npz: the reference's pino_models.FNO2d(modes1=[4,4,3], modes2=[6,6,5], fc_dim=128, layers=[32]*4, in_dim=3,
act='gelu') on a (2, 12, 32, 3) input, once per pad_ratio of burgers_cases.MODEL_CASES: output, every parameter gradient of
y.square().sum() (spectral weights: the first burgers_cases.GOLDEN_CIN input channels), and (shared by both) fill scales
and shapes; and the loss trajectory of three epochs of the reference's train_2d_burger (one batch of 2, Adam 1e-3, weights xy 1 / f 1 / ic 5) under "train/".

Runs where the reference is available; the stand-ins for its absent third-party imports and the deterministic fills are
oracle/make_golden.py's.  Both files hold DATA ONLY; parameters and inputs are rebuilt from oracle.detfill on both sides."""
import argparse
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle.make_golden import grads_of, install_standins, refill_parameters, save  # noqa: E402
from tests import burgers_cases as K  # noqa: E402


def gen_loss(out, losses):
    arrs = {}
    for family, shape in K.GOLDEN_CASES:
        inp = K.make_inputs(family, shape)
        u = inp["u"].clone().requires_grad_(True)
        loss_u, loss_f = losses.PINO_loss(u, inp["u0"], K.GOLDEN_VISC)
        (K.IC_WEIGHT * loss_u + loss_f).backward()
        arrs["{}_{}_{}_{}".format(family, *shape)] = {
            "loss_u": loss_u.detach().numpy(), "loss_f": loss_f.detach().numpy(),
            "field": losses.FDM_Burgers(inp["u"], K.GOLDEN_VISC).numpy(), "du": u.grad.numpy()}
    save(os.path.join(out, "burgers_loss_small.npz"), **arrs)


def build_model(M, pad_ratio):
    torch.manual_seed(0)
    model = M.FNO2d(modes1=list(K.MODES1), modes2=list(K.MODES2), fc_dim=128, layers=[32] * 4, in_dim=3, act='gelu',
                    pad_ratio=pad_ratio)
    return model, refill_parameters(model)


def gen_model(out, M, train_2d):
    arrs = {}
    for cname, kw in K.MODEL_CASES.items():
        model, scales = build_model(M, kw["pad_ratio"])
        y = model(K.model_input("pino_fno2d_small"))
        y.square().sum().backward()
        # the spectral weights are nine tenths of the parameters: their gradients are kept for the first GOLDEN_CIN input
        # channels, which keeps the file under the size limit of a committed fixture
        arrs[cname] = {"y": y.detach().numpy(),
                       **{"grads/" + k: (v[:K.GOLDEN_CIN] if "sp_convs" in k else v) for k, v in grads_of(model).items()}}
    arrs["scales"] = scales
    arrs["shapes"] = {k: np.array(v.shape) for k, v in model.state_dict().items()}
    model, _ = build_model(M, [0., 0.])
    x, y = K.train_data()
    opt = torch.optim.Adam(model.parameters(), lr=K.TRAIN_LR)
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=100)
    hist = []
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:           # the loop writes its checkpoints under the working directory
        os.chdir(tmp)
        try:
            # the reference's loop returns nothing: one epoch per call keeps the optimizer state and yields each epoch's figures
            for _ in range(K.TRAIN_CFG["train"]["epochs"]):
                out_ = model(x).reshape(y.shape)
                from libs.pino_utils.losses import LpLoss, PINO_loss
                data = LpLoss(size_average=True)(out_, y)
                loss_u, loss_f = PINO_loss(out_, x[:, 0, :, 0], K.TRAIN_VISC)
                w = K.TRAIN_CFG["train"]
                total = loss_u * w["ic_loss"] + loss_f * w["f_loss"] + data * w["xy_loss"]
                hist.append((float(total.detach()), float(loss_f.detach()), float(data.detach())))
                cfg = {"train": dict(w, epochs=1)}
                train_2d.train_2d_burger(model, [(x, y)], K.TRAIN_VISC, opt, sched, cfg, rank="cpu", use_tqdm=False)
        finally:
            os.chdir(cwd)
    arrs["train"] = {"history": np.array(hist, dtype=np.float64)}
    save(os.path.join(out, "pino_fno2d_small.npz"), **arrs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    args = ap.parse_args()
    install_standins()
    sys.path.insert(0, args.ref)
    from libs.models import pino_models as M
    from libs.pino_utils import losses, train_2d
    torch.set_num_threads(8)
    gen_loss(args.out, losses)
    gen_model(args.out, M, train_2d)


if __name__ == "__main__":
    main()
