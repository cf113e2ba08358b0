"""FNOBlocks with the reference surface (neuralop/models/fno_block.py:10-170): linear (bias-free 1x1 conv) skip, no norm, no
preactivation; with `use_mlp` the channel MLP and its soft-gating / identity skip (mlp.py:26-54, skip_connections.py:38-74)."""
import itertools

import torch
import torch.nn.functional as TF
from torch import nn

from ... import functional as F
from ... import layer_stack as LS
from .spectral_convolution import SpectralConv, _unsupported


def _resample(x, scales):
    """The skip branch on the resized grid of `output_scaling_factor` (fno_block.py:132-134 -> resample.py:6-56):
    linear / antialiased bicubic interpolation with aligned corners in 1-D / 2-D, Fourier zero-padding or truncation
    in 3-D.  Torch operations: this option has no HIP kernel (SpectralConv._torch_composition)."""
    old = x.shape[-len(scales):]
    new = tuple(int(round(s * r)) for s, r in zip(old, scales))
    if len(new) == 1:
        return TF.interpolate(x, size=new[0], mode='linear', align_corners=True)
    if len(new) == 2:
        return TF.interpolate(x, size=new, mode='bicubic', align_corners=True, antialias=True)
    dims = list(range(-len(new), 0))
    X = torch.fft.rfftn(x.float(), norm='forward', dim=dims)
    fsz = list(new[:-1]) + [new[-1] // 2 + 1]
    keep = [min(a, b) for a, b in zip(fsz, X.shape[-len(new):])]
    out = torch.zeros(x.shape[0], x.shape[1], *fsz, device=x.device, dtype=torch.cfloat)
    corners = [((None, m // 2), (-m // 2, None)) for m in keep[:-1]] + [((None, keep[-1]),)]
    for bounds in itertools.product(*corners):
        sl = (slice(None), slice(None)) + tuple(slice(*b) for b in bounds)
        out[sl] = X[sl]
    return torch.fft.irfftn(out, s=new, norm='forward', dim=dims)


class MLP(nn.Module):
    """The parameters of the reference's two-layer channel MLP (mlp.py:26-54: `fcs`, two 1x1 convolutions C -> H -> C, a GELU
    after EACH of them, :49).  Its arithmetic exists only as the engine kernel (functional.channel_mlp), which computes it
    together with the skip it is added to (FNOBlocks.forward)."""

    def __init__(self, in_channels, hidden_channels, n_dim=2):
        super().__init__()
        self.in_channels, self.out_channels, self.hidden_channels, self.n_layers = in_channels, in_channels, hidden_channels, 2
        Conv = getattr(nn, f'Conv{n_dim}d')
        self.fcs = nn.ModuleList([Conv(in_channels, hidden_channels, 1), Conv(hidden_channels, in_channels, 1)])

    def forward(self, x):
        return F.channel_mlp(x, torch.zeros_like(x), self.fcs[0].weight, self.fcs[0].bias, self.fcs[1].weight, self.fcs[1].bias)


class SoftGating(nn.Module):
    """x * w with w (1, C, 1, ..) initialised to ones, no bias (skip_connections.py:38-74)"""

    def __init__(self, in_features, out_features=None, n_dim=2, bias=False):
        super().__init__()
        if out_features is not None and in_features != out_features:
            raise ValueError(f"Got in_features={in_features} and out_features={out_features} "
                             "but these two must be the same for soft-gating")
        if bias:
            _unsupported("SoftGating(bias=True)")
        self.in_features, self.out_features = in_features, out_features
        self.weight = nn.Parameter(torch.ones(1, in_features, *(1,) * n_dim))
        self.bias = None

    def forward(self, x):
        return self.weight * x


class FNOBlocks(nn.Module):
    def __init__(self, in_channels, out_channels, n_modes, output_scaling_factor=None, n_layers=1,
                 incremental_n_modes=None, use_mlp=False, mlp_dropout=0, mlp_expansion=0.5,
                 non_linearity=TF.gelu, norm=None, ada_in_features=None, preactivation=False,
                 fno_skip='linear', mlp_skip='soft-gating', separable=False, factorization=None,
                 rank=1.0, SpectralConv=SpectralConv, joint_factorization=False,
                 fixed_rank_modes=False, implementation='factorized', decomposition_kwargs=dict(),
                 fft_norm='forward', **kwargs):
        super().__init__()
        if norm is not None:
            _unsupported(f"norm={norm!r}")
        if preactivation:
            _unsupported("preactivation=True")
        if fno_skip != 'linear':
            _unsupported(f"fno_skip={fno_skip!r}")
        if non_linearity is not TF.gelu:
            _unsupported("non_linearity other than F.gelu")
        if isinstance(n_modes, int):
            n_modes = [n_modes]
        self.n_modes = list(n_modes)
        self.n_dim = len(self.n_modes)
        self.in_channels, self.out_channels, self.n_layers = in_channels, out_channels, n_layers
        self.non_linearity = non_linearity
        self.fft_norm = fft_norm
        if output_scaling_factor is not None:           # fno_block.py:37-42
            if isinstance(output_scaling_factor, (float, int)):
                output_scaling_factor = [[float(output_scaling_factor)] * self.n_dim] * n_layers
            elif isinstance(output_scaling_factor[0], (float, int)):
                output_scaling_factor = [[s] * self.n_dim for s in output_scaling_factor]
        self.output_scaling_factor = output_scaling_factor
        self.convs = SpectralConv(in_channels, out_channels, self.n_modes,
                                  output_scaling_factor=output_scaling_factor,
                                  incremental_n_modes=incremental_n_modes, rank=rank, fft_norm=fft_norm,
                                  fixed_rank_modes=fixed_rank_modes, implementation=implementation,
                                  separable=separable, factorization=factorization,
                                  decomposition_kwargs=decomposition_kwargs,
                                  joint_factorization=joint_factorization, n_layers=n_layers)
        Conv = getattr(nn, f'Conv{self.n_dim}d')
        self.fno_skips = nn.ModuleList([Conv(in_channels, out_channels, kernel_size=1, bias=False)
                                        for _ in range(n_layers)])
        self.mlp = None
        if use_mlp:
            # the channel MLP exists only as the engine kernel: what the kernel does not cover is refused here
            hidden = int(round(out_channels * mlp_expansion))
            if in_channels != out_channels or (out_channels, hidden) not in F.CHANNEL_MLP_WIDTHS:
                _unsupported(f"use_mlp=True with (channels, mlp hidden width) = ({out_channels}, {hidden}); the channel-MLP kernel "
                             f"is built for {F.CHANNEL_MLP_WIDTHS}")
            if mlp_dropout > 0:
                _unsupported(f"mlp_dropout={mlp_dropout!r}")
            if str(mlp_skip).lower() not in ('soft-gating', 'identity'):
                if str(mlp_skip).lower() != 'linear':
                    raise ValueError(f"Got skip-connection type={mlp_skip!r}, expected one of 'soft-gating', 'linear', 'identity'.")
                _unsupported(f"mlp_skip={mlp_skip!r}")
            if output_scaling_factor is not None:
                _unsupported("use_mlp=True with output_scaling_factor")
            self.mlp = nn.ModuleList([MLP(out_channels, hidden, n_dim=self.n_dim) for _ in range(n_layers)])
            self.mlp_skips = nn.ModuleList([SoftGating(in_channels, out_channels, n_dim=self.n_dim)
                                            if str(mlp_skip).lower() == 'soft-gating' else nn.Identity()
                                            for _ in range(n_layers)])

    def gelu_after(self, index):
        return index < (self.n_layers - index)          # fno_block.py:149

    def pre_activation(self, x, index=0):
        """conv(x) + skip(x) of one block from this module's own parts (fno_block.py:123-147), before its activation"""
        y = self.convs(x, index)       # (first: with a channel MLP x has a third use, and autograd sums its gradients in this order)
        x_skip = self.fno_skips[index](x)
        if self.convs.output_scaling_factor is not None:
            x_skip = _resample(x_skip, self.output_scaling_factor[index])
        return y + x_skip

    ROUTES = (LS.FUSED, LS.TORCH)

    def stack(self, index=None):
        """the blocks without channel MLPs - or the Fourier part of block `index` alone - as layer_stack describes them"""
        convs, ls = self.convs, range(self.n_layers) if index is None else (index,)
        n, modes = len(ls), tuple(convs.half_n_modes)
        return LS.Stack((self.in_channels,) + (self.out_channels,) * n, lambda x, l: self.pre_activation(x, ls[l]),
                        F.default_gelu_mask(n) if index is None else 0, spec_ws=lambda l: convs.layer_weights(ls[l]),
                        uniform=convs.bias is not None and not convs.separable and convs.output_scaling_factor is None,
                        bias=convs.bias if index is None or convs.bias is None else convs.bias[index:index + 1], norm=self.fft_norm,
                        skip_ws=[self.fno_skips[l].weight for l in ls], modes=(modes,) * n, wle=(modes[-1],) * n, direct=(False,) * n)

    def _forward_mlp(self, x, index):
        """fno_block.py:137-169 with an MLP: u = gelu(conv(x) + skip(x)) on EVERY layer (:147-150), then
        gelu(fcs.1(gelu(fcs.0(u)))) + mlp_skip(x) - the skip takes the block's INPUT (:137) - and a GELU unless this is the
        last layer (:167-169).  The Fourier part is one fused engine layer (+ its GELU) where the block kernels cover the shape,
        the MLP part is functional.channel_mlp: without its kernel there is no MLP, so an uncovered shape raises."""
        F._require_cuda(x, "x")
        mlp, hidden = self.mlp[index], self.mlp[index].hidden_channels
        if not F.channel_mlp_supported(x, hidden):
            raise RuntimeError(f"fnoengine FNOBlocks(use_mlp=True): no channel-MLP kernel for input {tuple(x.shape)} {x.dtype} "
                               f"(float32, planes a multiple of 128 elements, (channels, hidden) in {F.CHANNEL_MLP_WIDTHS})")
        # one fused engine layer (spectral convolution + skip + bias, fixed-order weight-gradient reductions) where the block
        # kernels cover the shape.  Its GELU is a torch operation: the engine's block stacks end without activation unless a
        # projection follows (fno_model_plan_create), so `gelu_mask=1` on a one-layer stack is refused
        pre = LS.run(x, self.stack(index), self.ROUTES)
        u = self.non_linearity(pre)
        skip = self.mlp_skips[index]
        gate = skip.weight if isinstance(skip, SoftGating) else None
        return F.channel_mlp(u, x, mlp.fcs[0].weight, mlp.fcs[0].bias, mlp.fcs[1].weight, mlp.fcs[1].bias, gate,
                             gelu_out=index < self.n_layers - 1)

    def forward(self, x, index=0):
        """Unfused composition (one block on its own); FNO.forward uses the fused engine path."""
        if getattr(self, "mlp", None) is not None:      # (modules pickled before the channel MLP existed carry no `mlp`)
            return self._forward_mlp(x, index)
        x = self.pre_activation(x, index)
        if self.gelu_after(index):
            x = self.non_linearity(x)
        return x
