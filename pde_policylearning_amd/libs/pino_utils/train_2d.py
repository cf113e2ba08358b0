"""train_2d_burger with the reference surface (libs/pino_utils/train_2d.py:119-194): the Burgers PINO loop - model forward,
relative-L2 data loss, PINO_loss (initial condition + residual), backward, optimizer step - with the reference's loss
combination and checkpoint cadence - and train_2d_operator (:13-116), the Darcy PINO loop on functional.darcy_loss.  Model,
losses and (with trainer.FusedAdam) the update run on the engine."""
import math

import torch

from ... import functional as F
from .losses import LpLoss, PINO_loss
from .utils import save_checkpoint


def darcy_mollifier(mesh):
    """sin(pi x) sin(pi y) * 0.001 in float32 from the float32 mesh (S, S, 2), as train_2d.py:58 and eval_2d.py:27 build it"""
    return torch.sin(math.pi * mesh[..., 0]) * torch.sin(math.pi * mesh[..., 1]) * 0.001


def train_2d_operator(model, train_loader, optimizer, scheduler, config, rank=0, log=False, project='PINO-2d-default',
                      group='default', tags=['default'], use_tqdm=True, profile=False):
    """The Darcy PINO loop.  Returns [(train_loss, f_loss, data_loss)] per epoch, each weighted by batch size over
    len(train_loader.dataset) as the reference logs them.  log / project / group / tags (Weights & Biases) and profile are
    accepted and ignored.

    The reference function cannot run as written: it unpacks `data_ic, u, pde_ic` and then reads `x`, `y`, and `pred` when
    xy_loss is 0 (:68-80).  Its two evident intentions are built, chosen by what the loader yields:
      three-tuple (DarcyCombo)  the data term is LpLoss of model(data_ic) * mollifier against u - skipped, and reported as
                                zero, when xy_loss is 0; the equation term is darcy_loss of a second forward,
                                model(pde_ic) * pde_mol, with a = pde_ic[..., 0], on the equation grid.
      two-tuple (DarcyFlow)     one forward; both terms from one fused functional.darcy_loss call that takes y and the
                                mollifier.
    Each mollifier is built once, from the dataset's `mesh` / `pde_mesh`."""
    data_weight = config['train']['xy_loss']
    f_weight = config['train']['f_loss']
    model.train()
    myloss = LpLoss(size_average=True)
    pbar = range(config['train']['epochs'])
    if use_tqdm:
        from tqdm import tqdm
        pbar = tqdm(pbar, dynamic_ncols=True, smoothing=0.1)
    dataset = train_loader.dataset
    mollifier = darcy_mollifier(dataset.mesh).to(rank)
    pde_mol = darcy_mollifier(dataset.pde_mesh).to(rank) if hasattr(dataset, 'pde_mesh') else None
    history = []
    for e in pbar:
        train_loss = f_loss_sum = data_loss_sum = 0.0
        for batch in train_loader:
            optimizer.zero_grad()
            if len(batch) == 3:
                data_ic, u, pde_ic = (t.to(rank) for t in batch)
                if data_weight > 0:
                    pred = model(data_ic).squeeze(dim=-1) * mollifier
                    data_loss = myloss(pred, u)
                else:
                    data_loss = torch.zeros((), device=u.device)
                f_loss = F.darcy_loss(model(pde_ic), pde_ic[..., 0], mollifier=pde_mol)
            else:
                x, u = (t.to(rank) for t in batch)
                data_loss, f_loss = F.darcy_loss(model(x), x[..., 0], u, mollifier)
            loss = data_weight * data_loss + f_weight * f_loss
            loss.backward()
            optimizer.step()
            train_loss += loss.item() * u.shape[0]
            f_loss_sum += f_loss.item() * u.shape[0]
            data_loss_sum += data_loss.item() * u.shape[0]
        scheduler.step()
        history.append((train_loss / len(dataset), f_loss_sum / len(dataset), data_loss_sum / len(dataset)))
        if use_tqdm:
            pbar.set_description(f'Epoch: {e}, train loss: {history[-1][0]:.5f}, f_loss: {history[-1][1]:.5f}, '
                                 f'data loss: {history[-1][2]:.5f}')
    save_checkpoint(config['train']['save_dir'], config['train']['save_name'], model, optimizer)
    print('Done!')
    return history


def train_2d_burger(model, train_loader, v, optimizer, scheduler, config, rank=0, log=False, project='PINO-2d-default',
                    group='default', tags=['default'], use_tqdm=True):
    """Returns [(train_loss, train_pino, data_l2)] per epoch.  log / project / group / tags (the reference's Weights & Biases
    arguments) are accepted and ignored."""
    data_weight = config['train']['xy_loss']
    f_weight = config['train']['f_loss']
    ic_weight = config['train']['ic_loss']
    model.train()
    myloss = LpLoss(size_average=True)
    pbar = range(config['train']['epochs'])
    if use_tqdm:
        from tqdm import tqdm
        pbar = tqdm(pbar, dynamic_ncols=True, smoothing=0.1)
    history = []
    for e in pbar:
        model.train()
        train_pino = data_l2 = train_loss = 0.0
        for x, y in train_loader:
            x, y = x.to(rank), y.to(rank)
            out = model(x).reshape(y.shape)
            data_loss = myloss(out, y)
            loss_u, loss_f = PINO_loss(out, x[:, 0, :, 0], v)
            total_loss = loss_u * ic_weight + loss_f * f_weight + data_loss * data_weight
            optimizer.zero_grad()
            total_loss.backward()
            optimizer.step()
            data_l2 += data_loss.item()
            train_pino += loss_f.item()
            train_loss += total_loss.item()
        scheduler.step()
        data_l2 /= len(train_loader)
        train_pino /= len(train_loader)
        train_loss /= len(train_loader)
        history.append((train_loss, train_pino, data_l2))
        if use_tqdm:
            pbar.set_description(f'Epoch {e}, train loss: {train_loss:.5f} train f error: {train_pino:.5f}; '
                                 f'data l2 error: {data_l2:.5f}')
        if e % 100 == 0:
            save_checkpoint(config['train']['save_dir'], config['train']['save_name'].replace('.pt', f'_{e}.pt'), model, optimizer)
    save_checkpoint(config['train']['save_dir'], config['train']['save_name'], model, optimizer)
    print('Done!')
    return history
