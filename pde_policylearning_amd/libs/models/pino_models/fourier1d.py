"""FNO1d of the PINO models with the reference surface (libs/models/pino_models/fourier1d.py:6-62): fc0 (Linear in_dim -> width),
one SpectralConv1d + Conv1d(k=1) per layer with the activation between layers, fc1 / act / fc2.  Input (B, N, in_dim), output
(B, N, out_dim).  With act='gelu' the whole forward is engine calls (lifting, one spectral + pointwise layer per block chained
on pre-activations, projection head); any other activation keeps the spectral convolutions on the engine and the pointwise
parts as torch modules."""
import torch.nn.functional as TF
from torch import nn

from .... import layer_stack as LS
from .basics import SpectralConv1d

_ACTS = {"tanh": TF.tanh, "gelu": TF.gelu, "relu": TF.relu, "elu": TF.elu, "leaky_relu": TF.leaky_relu}     # utils.py:36-49


class FNO1d(nn.Module):
    def __init__(self, modes, width=32, layers=None, fc_dim=128, in_dim=2, out_dim=1, act='relu'):
        super().__init__()
        if act not in _ACTS:
            raise ValueError(f'{act} is not supported')
        self.modes1, self.width = modes, width
        if layers is None:
            layers = [width] * 4
        self.fc0 = nn.Linear(in_dim, layers[0])
        self.sp_convs = nn.ModuleList([SpectralConv1d(i, o, m) for i, o, m in zip(layers, layers[1:], self.modes1)])
        self.ws = nn.ModuleList([nn.Conv1d(i, o, 1) for i, o in zip(layers, layers[1:])])
        self.fc1 = nn.Linear(layers[-1], fc_dim)
        self.fc2 = nn.Linear(fc_dim, out_dim)
        self.act_name, self.act = act, _ACTS[act]

    ROUTES = (LS.CHAIN, LS.TORCH)

    def stack(self):
        uniform = self.act_name == "gelu" and len({w.in_channels for w in self.ws} | {w.out_channels for w in self.ws}) == 1
        return LS.conv_stack(self.sp_convs, self.ws, self.act,
                             [([sp.weights1], (sp.modes1,), sp.modes1) for sp in self.sp_convs] if uniform else None)

    def route(self, x, stack=None):
        """The rung the layers take for an input shaped like x (B, N, in_dim).  All of the engine or none of it: the chain
        needs the lifting and the projection head on their kernels too."""
        if not (x.is_cuda and x.dim() == 3):
            return LS.TORCH
        xt = x.permute(0, 2, 1)
        u = LS.probe(xt, self.fc0.out_features)
        ends = LS.lift_covered(xt, self.fc0) and LS.head_covered(u, self.fc1, self.fc2)
        return LS.route(u, stack or self.stack(), self.ROUTES if ends else (LS.TORCH,))

    def forward(self, x):
        stack = self.stack()
        rung = self.route(x, stack)
        if rung == LS.TORCH:
            u = LS.run(self.fc0(x).permute(0, 2, 1), stack, (rung,))
            return self.fc2(self.act(self.fc1(u.permute(0, 2, 1))))
        # chain: the activation behind layer i - 1 (fourier1d.py:55-56) is applied while layer i loads its input
        u = LS.run(LS.lift(x.permute(0, 2, 1), self.fc0), stack, (rung,))
        return LS.head(u, self.fc1, self.fc2).permute(0, 2, 1)
