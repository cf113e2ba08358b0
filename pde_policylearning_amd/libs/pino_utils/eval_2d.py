"""eval_darcy and eval_burgers with the reference surface (libs/pino_utils/eval_2d.py): per batch the relative-L2 test error
and the equation error, then their means and standard errors.  Both print the reference's two lines and also return
(mean_err, std_err, mean_f_err, std_f_err).  Model and losses run on the engine (functional.darcy_loss with the target and
the mollifier in one fused call; LpLoss + PINO_loss for Burgers)."""
import warnings

import numpy as np
import torch

from ... import functional as F
from .losses import LpLoss, PINO_loss
from .train_2d import darcy_mollifier


def _report(test_err, f_err):
    """a single batch has no standard error: nan, as numpy's ddof=1 gives it"""
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        mean_f_err, std_f_err = np.mean(f_err), np.std(f_err, ddof=1) / np.sqrt(len(f_err))
        mean_err, std_err = np.mean(test_err), np.std(test_err, ddof=1) / np.sqrt(len(test_err))
    print(f'==Averaged relative L2 error mean: {mean_err}, std error: {std_err}==\n'
          f'==Averaged equation error mean: {mean_f_err}, std error: {std_f_err}==')
    return float(mean_err), float(std_err), float(mean_f_err), float(std_f_err)


def _progress(dataloader, use_tqdm):
    if not use_tqdm:
        return dataloader
    from tqdm import tqdm
    return tqdm(dataloader, dynamic_ncols=True, smoothing=0.05)


def eval_darcy(model, dataloader, config, device, use_tqdm=True):
    model.eval()
    pbar = _progress(dataloader, use_tqdm)
    mollifier = darcy_mollifier(dataloader.dataset.mesh).to(device)
    f_val, test_err = [], []
    with torch.no_grad():
        for x, y in pbar:
            x, y = x.to(device), y.to(device)
            data_loss, f_loss = F.darcy_loss(model(x).reshape(y.shape), x[..., 0], y, mollifier)
            test_err.append(data_loss.item())
            f_val.append(f_loss.item())
            if use_tqdm:
                pbar.set_description(f'Equation error: {f_val[-1]:.5f}, test l2 error: {test_err[-1]}')
    return _report(test_err, f_val)


def eval_burgers(model, dataloader, v, config, device, use_tqdm=True):
    model.eval()
    myloss = LpLoss(size_average=True)
    test_err, f_err = [], []
    with torch.no_grad():
        for x, y in _progress(dataloader, use_tqdm):
            x, y = x.to(device), y.to(device)
            out = model(x).reshape(y.shape)
            data_loss = myloss(out, y)
            _, f_loss = PINO_loss(out, x[:, 0, :, 0], v)
            test_err.append(data_loss.item())
            f_err.append(f_loss.item())
    return _report(test_err, f_err)
