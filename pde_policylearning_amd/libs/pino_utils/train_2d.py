"""train_2d_burger with the reference surface (libs/pino_utils/train_2d.py:119-194): the Burgers PINO loop - model forward,
relative-L2 data loss, PINO_loss (initial condition + residual), backward, optimizer step - with the reference's loss
combination and checkpoint cadence.  Model, losses and (with trainer.FusedAdam) the update run on the engine.  The Darcy loop
train_2d_operator of the same file is not provided."""
from .losses import LpLoss, PINO_loss
from .utils import save_checkpoint


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
