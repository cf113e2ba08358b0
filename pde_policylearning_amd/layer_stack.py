"""The route of a stack of Fourier layers  y_l = SpectralConv(a_l) + Conv_{k=1}(a_l) + bias_l,  a_{l+1} = act(y_l)  through the
engine, stated once.  A model describes its stack (`Stack`), names the rungs it implements (`allowed`)
and calls `run`; `route` answers which rung that is without launching anything.  `lift` and `head` state the same choice for the
two ends of a model, `clear_direct_grads` is what a forward on an autograd route owes a direct-write bucket."""
import typing

import torch
import torch.nn.functional as TF
from torch import nn

from . import functional as F

# fused: the whole stack as ONE engine block stack (functional.fno_blocks).  chain: one functional.spectral_pointwise_layer per
# layer on PRE-activation tensors.  addend: per layer the model's own spectral convolution as the addend of the engine's pointwise
# mix, the activation a torch operation.  torch: per layer the model's own torch modules around its engine spectral convolution.
FUSED, CHAIN, ADDEND, TORCH = RUNGS = ("fused", "chain", "addend", "torch")


class Stack(typing.NamedTuple):
    """One stack of Fourier layers.  A model whose layers differ in width or kept modes, or that has separable weights, a
    resized grid, no bias or another activation than GELU says `uniform=False`: only the last two rungs are open to it, and
    the fields from spec_ws to direct may stay None."""
    widths: tuple                       # channels in front of layer 0, behind layer 0, ... (n_layers + 1 entries)
    torch_layer: typing.Callable        # (x, l) -> layer l from the model's own torch modules, before the activation of `act_mask`
    act_mask: int = 0                   # bit l set: `act` follows layer l
    act: typing.Callable = TF.gelu
    uniform: bool = False
    spec_ws: typing.Callable = None     # l -> the corner weights of layer l in the engine's order (read when a rung runs)
    skip_ws: typing.Sequence = None     # per layer the 1x1 weight
    bias: typing.Any = None             # per layer one bias row (a list), or one (n_layers, C, 1..) tensor
    modes: typing.Sequence = None       # per layer the kept modes
    norm: str = "backward"
    wle: typing.Sequence = None         # per layer the stored last-dim extent of the weights (weight_last_extent)
    direct: typing.Sequence = None      # per layer: spectral-weight gradients are written into their existing .grad storage
    spectral: typing.Callable = None    # (x, l) -> the model's own spectral convolution of layer l (the addend rung)

    def act_in(self, l):
        return l > 0 and bool(self.act_mask >> (l - 1) & 1)


def probe(x, channels, grid=None):
    """a (B, channels) + grid view of x's memory for the shape predicates and route(): no tensor of the hidden shape is made"""
    shape = (x.shape[0], channels) + tuple(x.shape[2:] if grid is None else grid)
    return x if shape == tuple(x.shape) else x.detach().as_strided(shape, (0,) * len(shape))


def conv_stack(sp_convs, ws, act, engine_calls=None, norm="backward"):
    """The Stack of modules: per layer a spectral convolution beside a Conv1d(k=1), `act` between the layers (PINO models, RNO).
    engine_calls: per layer (corner weights in engine order, kept modes, stored last extent); given, the stack is uniform."""
    def torch_layer(x, l):
        return sp_convs[l](x) + ws[l](x.reshape(x.shape[0], ws[l].in_channels, -1)).view(x.shape[0], ws[l].out_channels, *x.shape[2:])
    s = Stack((ws[0].in_channels,) + tuple(w.out_channels for w in ws), torch_layer, (1 << (len(ws) - 1)) - 1, act,
              skip_ws=[w.weight for w in ws], bias=[w.bias for w in ws], spectral=lambda x, l: sp_convs[l](x))
    if engine_calls is None:
        return s
    return s._replace(uniform=True, spec_ws=lambda l: engine_calls[l][0], modes=[c[1] for c in engine_calls], norm=norm,
                      wle=[c[2] for c in engine_calls], direct=[getattr(sp, "_direct_grads", False) for sp in sp_convs])


_COVERS = {
    FUSED: lambda x, s: (s.uniform and len(set(s.modes)) == 1 and all(e == s.modes[0][-1] for e in s.wle)
                         and F.blocks_supported(x, len(s.modes), s.modes[0], s.norm, s.act_mask)),
    CHAIN: lambda x, s: s.uniform and all(F.spectral_layer_supported(x, 2 ** (len(m) - 1), m, s.norm, e, s.act_in(l))
                                          for l, (m, e) in enumerate(zip(s.modes, s.wle))),
    ADDEND: lambda x, s: s.spectral is not None and any(a == b and F.pointwise_supported(probe(x, a))
                                                        for a, b in zip(s.widths, s.widths[1:])),
    TORCH: lambda x, s: True}


def route(x, stack, allowed=RUNGS):
    """The first rung of `allowed` that covers a (B, widths[0], ...) input shaped like x, or None.  The predicates read shape,
    dtype and device and are asked on every call (functional keeps the engine's answers per plan), so no launch, no tensor."""
    x0 = probe(x, stack.widths[0])
    return next((r for r in RUNGS if r in allowed and _COVERS[r](x0, stack)), None)


def run(x, stack, allowed=RUNGS):
    """The stack applied to x by the rung route() names; raises when none of `allowed` covers the input."""
    s, n, rung = stack, len(stack.widths) - 1, route(x, stack, allowed)
    if rung is None:
        raise RuntimeError(f"fnoengine layer stack: none of the routes {allowed} covers input {tuple(x.shape)} {x.dtype} on {x.device}")
    if rung == FUSED:
        bias = (s.bias.reshape(n, -1) if torch.is_tensor(s.bias) else s.bias[0].view(1, -1) if n == 1 else torch.stack(list(s.bias)))
        return F.fno_blocks(x, list(s.skip_ws), [w for l in range(n) for w in s.spec_ws(l)], bias, s.modes[0], s.norm,
                            gelu_mask=s.act_mask, direct_grads=all(s.direct))
    for l in range(n):
        if rung == CHAIN:
            # layer l applies layer l - 1's GELU while it loads its input; its backward folds gelu' and the two-branch sum in
            bias = s.bias[l].reshape(-1) if torch.is_tensor(s.bias) else s.bias[l]
            x = F.spectral_pointwise_layer(x, s.spec_ws(l), s.modes[l], s.norm, s.skip_ws[l], bias, input_gelu=s.act_in(l),
                                           weight_last_extent=s.wle[l], direct_grads=s.direct[l])
        elif rung == ADDEND and s.widths[l] == s.widths[l + 1] and F.pointwise_supported(x):
            x = F.pointwise_conv_add(x, s.skip_ws[l], s.bias[l], addend=s.spectral(x, l))
        else:
            x = s.torch_layer(x, l)
        if s.act_mask >> l & 1 and (rung != CHAIN or l == n - 1):      # (the chain applies its inner activations on load)
            x = s.act(x)
    return x


def lift_covered(xc, fc):
    return F.lifting_supported(xc, fc.weight.shape[0])


def head_covered(x, fc1, fc2, act="gelu"):
    return F.projection_supported(x, fc1.weight.shape[0], fc2.weight.shape[0], act)


def lift(xc, fc):
    """fc (a Linear, whose torch form is channels-last, or a 1x1 convolution) applied to the channels-first xc: the engine's
    lifting kernels where they cover the shape, the torch module otherwise; channels-first either way."""
    if lift_covered(xc, fc):
        return F.lifting(xc, fc.weight, fc.bias)
    return fc(xc.movedim(1, -1)).movedim(-1, 1) if isinstance(fc, nn.Linear) else fc(xc)


def head(x, fc1, fc2, act="gelu"):
    """fc2(act(fc1(x))) on the channels-first x: the engine's projection kernels (act 'gelu' or 'relu') where they cover the
    shape, the torch modules otherwise; channels-first either way."""
    if head_covered(x, fc1, fc2, act):
        return F.projection_head(x, fc1.weight, fc1.bias, fc2.weight, fc2.bias, act=act)
    fn = getattr(TF, act)
    return fc2(fn(fc1(x.movedim(1, -1)))).movedim(-1, 1) if isinstance(fc1, nn.Linear) else fc2(fn(fc1(x)))


def clear_direct_grads(module):
    """A direct-write bucket (trainer.FlatGradBucket(direct_module=...)) does not clear `module`'s gradients: it expects the
    engine to overwrite them.  A forward that hands its gradients to autograd, which accumulates, clears them here."""
    if getattr(module, "_direct_grads", False) and torch.is_grad_enabled():
        for p in module.parameters():
            if p.grad is not None:
                p.grad.zero_()
