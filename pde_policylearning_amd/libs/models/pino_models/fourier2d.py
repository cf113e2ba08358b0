"""FNO2d of the PINO models with the reference surface (libs/models/pino_models/fourier2d.py:6-87): fc0 (Linear in_dim ->
layers[0]), one SpectralConv2d + Conv1d(k=1) per layer with the activation between layers, zero padding added once before the
layers and cropped once after them (torch operations), and the three-layer head fc1 / act / fc2 / act / fc3.  Input
(B, X, Y, in_dim), output (B, X, Y, out_dim).  This is the model train_2d_burger trains (libs/pino_utils/train_2d.py).

With act='gelu', one width for every layer and shapes the kernels take, everything between the input and the head is engine
calls: lifting, then one spectral + pointwise layer per block chained on pre-activations.  The head maps
layers[-1] -> fc_dim -> layers[-1] -> out_dim; the engine's projection head ends in at most four channels, so it does not
cover the middle map and the head runs as torch modules on either route.  Any other configuration keeps the spectral
convolutions on the engine and the pointwise parts as torch modules.  There is no CPU path.

`layers=None`: the reference stores [width] * (len(modes1) + 1) in self.layers and then indexes the ARGUMENT (fourier2d.py:38,
48-50), which raises TypeError; the evidently intended default is what is built here."""
import torch.nn.functional as TF
from torch import nn

from .... import layer_stack as LS
from .basics import SpectralConv2d
from .fourier1d import _ACTS


def add_padding2(x, num_pad1, num_pad2):
    """zeros behind / in front of the last two dimensions (libs/models/pino_models/utils.py:12-17)"""
    if max(num_pad1) > 0 or max(num_pad2) > 0:
        return TF.pad(x, (num_pad2[0], num_pad2[1], num_pad1[0], num_pad1[1]), 'constant', 0.)
    return x


def remove_padding2(x, num_pad1, num_pad2):
    """the reference's crop (utils.py:28-33), end indices -num_pad[1] as written there"""
    if max(num_pad1) > 0 or max(num_pad2) > 0:
        return x[..., num_pad1[0]:-num_pad1[1], num_pad2[0]:-num_pad2[1]]
    return x


class FNO2d(nn.Module):
    def __init__(self, modes1, modes2, width=64, fc_dim=128, layers=None, in_dim=3, out_dim=1, act='gelu', pad_ratio=[0., 0.]):
        super().__init__()
        if act not in _ACTS:
            raise ValueError(f'{act} is not supported')
        if isinstance(pad_ratio, float):
            pad_ratio = [pad_ratio, pad_ratio]
        else:
            assert len(pad_ratio) == 2, 'Cannot add padding in more than 2 directions'
        self.modes1, self.modes2, self.pad_ratio = modes1, modes2, list(pad_ratio)
        self.layers = [width] * (len(modes1) + 1) if layers is None else layers
        self.fc0 = nn.Linear(in_dim, self.layers[0])
        self.sp_convs = nn.ModuleList([SpectralConv2d(i, o, m1, m2)
                                       for i, o, m1, m2 in zip(self.layers, self.layers[1:], self.modes1, self.modes2)])
        self.ws = nn.ModuleList([nn.Conv1d(i, o, 1) for i, o in zip(self.layers, self.layers[1:])])
        self.fc1 = nn.Linear(self.layers[-1], fc_dim)
        self.fc2 = nn.Linear(fc_dim, self.layers[-1])
        self.fc3 = nn.Linear(self.layers[-1], out_dim)
        self.act_name, self.act = act, _ACTS[act]

    def _pads(self, size_1, size_2):
        if max(self.pad_ratio) > 0:
            return [round(i * size_1) for i in self.pad_ratio], [round(i * size_2) for i in self.pad_ratio]
        return [0, 0], [0, 0]

    ROUTES = (LS.CHAIN, LS.TORCH)

    def stack(self):
        uniform = self.act_name == "gelu" and len(set(self.layers)) == 1
        return LS.conv_stack(self.sp_convs, self.ws, self.act, [([sp.weights1, sp.weights2], (sp.modes1, sp.modes2), sp.modes2)
                                                                for sp in self.sp_convs] if uniform else None)

    def route(self, x, stack=None):
        """The rung the layers take for an input shaped like x (B, X, Y, in_dim); they see the PADDED grid.  All of the engine
        up to the head or none of it: the chain needs the lifting on its kernels too."""
        if not (x.is_cuda and x.dim() == 4):
            return LS.TORCH
        xt = x.permute(0, 3, 1, 2)
        p1, p2 = self._pads(x.shape[1], x.shape[2])
        u = LS.probe(xt, self.layers[0], (x.shape[1] + sum(p1), x.shape[2] + sum(p2)))
        return LS.route(u, stack or self.stack(), self.ROUTES if LS.lift_covered(xt, self.fc0) else (LS.TORCH,))

    def _head(self, x):
        return self.fc3(self.act(self.fc2(self.act(self.fc1(x)))))

    def forward(self, x):
        if not x.is_cuda:
            raise RuntimeError(f"fnoengine FNO2d: the input must live on the GPU (got {x.device}); the engine has no CPU path")
        num_pad1, num_pad2 = self._pads(x.shape[1], x.shape[2])
        stack = self.stack()
        rung = self.route(x, stack)
        u = LS.lift(x.permute(0, 3, 1, 2), self.fc0) if rung == LS.CHAIN else self.fc0(x).permute(0, 3, 1, 2)
        u = add_padding2(u, num_pad1, num_pad2)
        # chain: the activation behind layer i - 1 (fourier2d.py:78-79) is applied while layer i loads its input
        u = LS.run(u, stack, (rung,))
        return self._head(remove_padding2(u, num_pad1, num_pad2).permute(0, 2, 3, 1))
