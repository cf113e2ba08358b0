"""FNO / FNO1d / FNO2d / FNO3d with the reference constructor surface (neuralop/models/tfno.py:
Lifting :11-20, Projection :23-38, FNO :107-211, FNO1d :222-340, FNO2d :342-458, FNO3d :467-580).
forward() runs the whole model in the HIP engine (functional.fno_model); with `use_mlp` it runs layer by layer, every block
as one fused Fourier layer and one channel-MLP kernel."""
import torch
import torch.nn.functional as TF
from torch import nn

from ... import functional as F
from ... import layer_stack as LS
from .fno_block import FNOBlocks
from .padding import DomainPadding
from .spectral_convolution import SpectralConv, _unsupported


class Lifting(nn.Module):
    def __init__(self, in_channels, out_channels, n_dim=2):
        super().__init__()
        self.in_channels, self.out_channels = in_channels, out_channels
        self.fc = getattr(nn, f'Conv{n_dim}d')(in_channels, out_channels, 1)

    def forward(self, x):
        return self.fc(x)


class Projection(nn.Module):
    def __init__(self, in_channels, out_channels, hidden_channels=None, n_dim=2, non_linearity=TF.gelu):
        super().__init__()
        self.in_channels, self.out_channels = in_channels, out_channels
        self.hidden_channels = in_channels if hidden_channels is None else hidden_channels
        self.non_linearity = non_linearity
        Conv = getattr(nn, f'Conv{n_dim}d')
        self.fc1 = Conv(in_channels, hidden_channels, 1)
        self.fc2 = Conv(hidden_channels, out_channels, 1)

    def forward(self, x):
        return self.fc2(self.non_linearity(self.fc1(x)))


class FNO(nn.Module):
    """neuralop.models.FNO (tfno.py:107-211).

    `domain_padding=f` (with `domain_padding_mode` 'one-sided' or 'symmetric') zero-pads the lifted field by round(f * r)
    entries per grid axis, runs the Fourier blocks on the extended grid and crops before the projection, as the reference
    does on square and cubic grids.  On a grid whose axes get different amounts the reference's pad and unpad disagree
    ((32, 64) at 0.25 -> (48, 72) -> (40, 56); (8, 8, 12) -> (11, 10, 14) -> (9, 8, 11); (2, 40) unpads to an empty tensor) and
    its model returns the wrong shape; here every axis is padded and cropped by its own amount, so the output has the input's
    grid (padding.DomainPadding).  Padding cannot be combined with `output_scaling_factor`."""

    def __init__(self, n_modes, hidden_channels, in_channels=3, out_channels=1, lifting_channels=256,
                 projection_channels=256, n_layers=4, output_scaling_factor=None,
                 incremental_n_modes=None, use_mlp=False, mlp_dropout=0, mlp_expansion=0.5,
                 non_linearity=TF.gelu, norm=None, preactivation=False, fno_skip='linear',
                 mlp_skip='soft-gating', separable=False, factorization=None, rank=1.0,
                 joint_factorization=False, fixed_rank_modes=False, implementation='factorized',
                 decomposition_kwargs=dict(), domain_padding=None, domain_padding_mode='one-sided',
                 fft_norm='forward', SpectralConv=SpectralConv, **kwargs):
        super().__init__()
        if domain_padding is not None and domain_padding > 0:      # a scalar, as in the reference (tfno.py:158)
            if output_scaling_factor is not None:
                raise NotImplementedError("fnoengine FNO: domain_padding together with output_scaling_factor is not supported "
                                          "(the resized blocks are torch compositions)")
            self.domain_padding = DomainPadding(domain_padding=domain_padding, padding_mode=domain_padding_mode)
        else:
            self.domain_padding = None
        self.domain_padding_mode = domain_padding_mode
        self.n_dim = len(n_modes)
        self.n_modes = tuple(n_modes)
        self.hidden_channels = hidden_channels
        self.lifting_channels = lifting_channels        # stored, unused (tfno.py:191)
        self.projection_channels = projection_channels
        self.in_channels, self.out_channels, self.n_layers = in_channels, out_channels, n_layers
        self.fft_norm = fft_norm
        self.non_linearity = non_linearity
        self.fno_blocks = FNOBlocks(
            in_channels=hidden_channels, out_channels=hidden_channels, n_modes=self.n_modes,
            output_scaling_factor=output_scaling_factor, use_mlp=use_mlp, mlp_dropout=mlp_dropout,
            mlp_expansion=mlp_expansion, non_linearity=non_linearity, norm=norm,
            preactivation=preactivation, fno_skip=fno_skip, mlp_skip=mlp_skip,
            incremental_n_modes=incremental_n_modes, rank=rank, fft_norm=fft_norm,
            fixed_rank_modes=fixed_rank_modes, implementation=implementation, separable=separable,
            factorization=factorization, decomposition_kwargs=decomposition_kwargs,
            joint_factorization=joint_factorization, SpectralConv=SpectralConv, n_layers=n_layers)
        self.lifting = Lifting(in_channels, hidden_channels, n_dim=self.n_dim)
        self.projection = Projection(hidden_channels, out_channels, hidden_channels=projection_channels,
                                     non_linearity=non_linearity, n_dim=self.n_dim)

    def engine_args(self):
        blk = self.fno_blocks
        L = self.n_layers
        skip_ws = [blk.fno_skips[l].weight for l in range(L)]
        spec_ws = [w for l in range(L) for w in blk.convs.layer_weights(l)]    # sliced under incremental_n_modes
        return dict(lift_w=self.lifting.fc.weight, lift_b=self.lifting.fc.bias, skip_ws=skip_ws,
                    spec_ws=spec_ws, spec_bias=blk.convs.bias,
                    w1=self.projection.fc1.weight, b1=self.projection.fc1.bias,
                    w2=self.projection.fc2.weight, b2=self.projection.fc2.bias,
                    modes=blk.convs.half_n_modes, norm=self.fft_norm)

    def fused_supported(self, x):
        """Shapes the whole-model fused kernels cover (fno_model_plan_create): hidden width 32/64,
        <= 4 input / output channels, projection_channels 256, and either rows that tile the 128 / 256-pixel workgroup tile
        (last dim 32, 64, 128, 256) or "loose rows" (any last dim in 32..320 on planes that tile by 128 pixels: 96 x 96,
        160 x 160, 192 x 192 grids ...; split-precision GEMM mode)."""
        if getattr(self, "domain_padding", None) is not None:
            return False           # the whole-model plan knows no padding: lifting, pad, block stack, crop, projection (forward)
        if self.fno_blocks.convs.separable or self.fno_blocks.convs.output_scaling_factor is not None:
            return False           # torch compositions (SpectralConv._torch_composition): layer by layer
        if getattr(self.fno_blocks, "mlp", None) is not None:
            return False           # the whole-model plan knows no channel MLP: layer by layer (FNOBlocks._forward_mlp)
        if not (self.hidden_channels in (32, 64) and self.in_channels <= 4 and self.out_channels <= 4
                and self.projection_channels == 256 and x.is_cuda and F.row_tiling(tuple(x.shape[2:])) is not None
                and (not x.requires_grad or self.in_channels <= 4)):
            return False
        # the engine has the last word (e.g. 256-pixel tiles with many kept modes do not fit LDS)
        gelu_mask = F.default_gelu_mask(self.n_layers)
        return F.model_plan_available(self.n_dim, self.in_channels, self.hidden_channels, self.out_channels,
                                      self.projection_channels, self.n_layers, tuple(x.shape[2:]),
                                      tuple(m // 2 for m in self.n_modes), self.fft_norm, gelu_mask, x.device)

    def forward(self, x):
        sliced = self.fno_blocks.convs.incremental_n_modes is not None
        if self.fused_supported(x) and not (sliced and getattr(self, "_direct_grads", False)):
            # direct_grads: set by trainer.FlatGradBucket(model, direct=True); the engine then writes
            # parameter gradients straight into the flat bucket (one use of each parameter per step; sliced weights
            # under incremental_n_modes are copies, so that combination takes the composition below)
            return F.fno_model(x, direct_grads=getattr(self, "_direct_grads", False),
                               overlap=getattr(self, "_grad_overlap", None), **self.engine_args())
        # other widths / grids, domain padding (tfno.py:195-211), channel MLPs: every gradient through autograd.  Without
        # padding and MLPs lifting and projection are torch modules and the blocks take the last rung
        LS.clear_direct_grads(self)
        pad = getattr(self, "domain_padding", None)      # (modules pickled before the option existed have no such attribute)
        mlp = getattr(self.fno_blocks, "mlp", None) is not None
        engine = pad is not None or mlp
        if engine:
            F._require_cuda(x, "x")
        x = LS.lift(x, self.lifting.fc) if engine else self.lifting(x)
        x = x if pad is None else pad.pad(x)
        if mlp:                                # blocks with a channel MLP route their own Fourier part (FNOBlocks._forward_mlp)
            for l in range(self.n_layers):
                x = self.fno_blocks(x, l)
        else:
            x = LS.run(x, self.fno_blocks.stack(), self.fno_blocks.ROUTES if engine else (LS.TORCH,))
        x = x if pad is None else pad.unpad(x)
        return LS.head(x, self.projection.fc1, self.projection.fc2) if engine else self.projection(x)


class FNO2d(FNO):
    def __init__(self, n_modes_height, n_modes_width, hidden_channels, in_channels=3, out_channels=1,
                 lifting_channels=256, projection_channels=256, n_layers=4, output_scaling_factor=None,
                 incremental_n_modes=None, non_linearity=TF.gelu, use_mlp=False, mlp_dropout=0,
                 mlp_expansion=0.5, norm=None, skip='soft-gating', separable=False, preactivation=False,
                 factorization=None, rank=1.0, joint_factorization=False, fixed_rank_modes=False,
                 implementation='factorized', decomposition_kwargs=dict(), domain_padding=None,
                 domain_padding_mode='one-sided', fft_norm='forward', **kwargs):
        # `skip` is accepted and ignored exactly as in the reference (tfno.py:449 -> **kwargs :131)
        super().__init__(
            n_modes=(n_modes_height, n_modes_width), hidden_channels=hidden_channels,
            in_channels=in_channels, out_channels=out_channels, lifting_channels=lifting_channels,
            projection_channels=projection_channels, n_layers=n_layers, output_scaling_factor=None,
            non_linearity=non_linearity, use_mlp=use_mlp, mlp_dropout=mlp_dropout,
            mlp_expansion=mlp_expansion, incremental_n_modes=incremental_n_modes, norm=norm,
            separable=separable, preactivation=preactivation, factorization=factorization, rank=rank,
            joint_factorization=joint_factorization, fixed_rank_modes=fixed_rank_modes,
            implementation=implementation, decomposition_kwargs=decomposition_kwargs,
            domain_padding=domain_padding, domain_padding_mode=domain_padding_mode, fft_norm=fft_norm)
        self.n_modes_height, self.n_modes_width = n_modes_height, n_modes_width


class FNO3d(FNO):
    def __init__(self, n_modes_height, n_modes_width, n_modes_depth, hidden_channels, in_channels=3,
                 out_channels=1, lifting_channels=256, projection_channels=256, n_layers=4,
                 output_scaling_factor=None, incremental_n_modes=None, non_linearity=TF.gelu,
                 use_mlp=False, mlp_dropout=0, mlp_expansion=0.5, norm=None, skip='soft-gating',
                 separable=False, preactivation=False, factorization=None, rank=1.0,
                 joint_factorization=False, fixed_rank_modes=False, implementation='factorized',
                 decomposition_kwargs=dict(), domain_padding=None, domain_padding_mode='one-sided',
                 fft_norm='forward', **kwargs):
        super().__init__(
            n_modes=(n_modes_height, n_modes_width, n_modes_depth), hidden_channels=hidden_channels,
            in_channels=in_channels, out_channels=out_channels, lifting_channels=lifting_channels,
            projection_channels=projection_channels, n_layers=n_layers, output_scaling_factor=None,
            non_linearity=non_linearity, use_mlp=use_mlp, mlp_dropout=mlp_dropout,
            mlp_expansion=mlp_expansion, incremental_n_modes=incremental_n_modes, norm=norm,
            separable=separable, preactivation=preactivation, factorization=factorization, rank=rank,
            joint_factorization=joint_factorization, fixed_rank_modes=fixed_rank_modes,
            implementation=implementation, decomposition_kwargs=decomposition_kwargs,
            domain_padding=domain_padding, domain_padding_mode=domain_padding_mode, fft_norm=fft_norm)
        self.n_modes_height, self.n_modes_width, self.n_modes_depth = n_modes_height, n_modes_width, n_modes_depth


class FNO1d(FNO):
    """neuralop.models.FNO1d (tfno.py:222-340) on (B, in_channels, N) grids.  One-dimensional models exist only on the engine's
    1-D kernels (k_spec1d.h): hidden width 32 or 64, N a multiple of 128 in [128, 8192], at most 64 kept bins.  forward() is
    the lifting, one spectral + pointwise layer per block chained on PRE-activation tensors (the GELU behind block l - 1 is
    applied while block l loads its input), and the projection head."""

    WIDTHS = (32, 64)

    def __init__(self, n_modes_height, hidden_channels, in_channels=3, out_channels=1, lifting_channels=256,
                 projection_channels=256, incremental_n_modes=None, n_layers=4, output_scaling_factor=None,
                 non_linearity=TF.gelu, use_mlp=False, mlp_dropout=0, mlp_expansion=0.5, norm=None,
                 skip='soft-gating', separable=False, preactivation=False, factorization=None, rank=1.0,
                 joint_factorization=False, fixed_rank_modes=False, implementation='factorized',
                 decomposition_kwargs=dict(), domain_padding=None, domain_padding_mode='one-sided',
                 fft_norm='forward', **kwargs):
        if hidden_channels not in self.WIDTHS:
            raise NotImplementedError(f"fnoengine FNO1d: hidden_channels={hidden_channels}; the one-dimensional kernels are built "
                                      f"for hidden widths {self.WIDTHS}")
        for name, on in (("use_mlp=True", use_mlp), ("separable=True", separable),
                         ("output_scaling_factor", output_scaling_factor is not None)):
            if on:
                raise NotImplementedError(f"fnoengine FNO1d: {name} has no one-dimensional kernel")
        super().__init__(
            n_modes=(n_modes_height,), hidden_channels=hidden_channels,
            in_channels=in_channels, out_channels=out_channels, lifting_channels=lifting_channels,
            projection_channels=projection_channels, n_layers=n_layers, output_scaling_factor=None,
            non_linearity=non_linearity, use_mlp=False, mlp_dropout=mlp_dropout,
            mlp_expansion=mlp_expansion, incremental_n_modes=incremental_n_modes, norm=norm,
            separable=False, preactivation=preactivation, factorization=factorization, rank=rank,
            joint_factorization=joint_factorization, fixed_rank_modes=fixed_rank_modes,
            implementation=implementation, decomposition_kwargs=decomposition_kwargs,
            domain_padding=domain_padding, domain_padding_mode=domain_padding_mode, fft_norm=fft_norm)
        self.n_modes_height = n_modes_height

    def fused_supported(self, x):
        """the whole-model plan (fno_model_plan_create) has no one-dimensional form: forward() below is the layer chain"""
        return False

    def _hidden_length(self, n):
        """the length the blocks run on: N, or N with its domain padding (what the 1-D kernels' shape rule applies to)"""
        pad = getattr(self, "domain_padding", None)
        return n if pad is None else pad.padded_resolution((n,))[0]

    ROUTES = (LS.CHAIN,)

    def forward(self, x):
        F._require_cuda(x, "x")
        stack = self.fno_blocks.stack()
        pad = getattr(self, "domain_padding", None)      # (modules pickled before the option existed have no such attribute)
        ok = x.dim() == 3 and x.shape[1] == self.in_channels
        if not (ok and LS.route(LS.probe(x, self.hidden_channels, (self._hidden_length(x.shape[2]),)), stack, self.ROUTES)):
            padded = "" if pad is None or x.dim() != 3 else f" padded to N = {self._hidden_length(x.shape[2])}"
            raise RuntimeError(f"fnoengine FNO1d: no one-dimensional kernel for input {tuple(x.shape)}{padded} with {stack.modes[0][0]} kept bins "
                               f"(needs (B, {self.in_channels}, N), N a multiple of 128 in [128, 8192], at most 64 kept bins"
                               f"{'; with domain padding the rule applies to the padded N' if pad is not None else ''})")
        LS.clear_direct_grads(self)           # this forward hands every gradient to autograd (as FNO.forward's layer routes do)
        u = LS.lift(x, self.lifting.fc)
        u = LS.run(u if pad is None else pad.pad(u), stack, self.ROUTES)      # (only a one-layer stack ends on an activation)
        u = u if pad is None else pad.unpad(u)
        return LS.head(u, self.projection.fc1, self.projection.fc2)


def _with_defaults(new_name, cls, **defaults):
    """A subclass of `cls` whose constructor has other default values (the role of tfno.py:594-615)."""
    def __init__(self, *args, **kwargs):
        for k, v in defaults.items():
            kwargs.setdefault(k, v)
        cls.__init__(self, *args, **kwargs)
    return type(new_name, (cls,), {"__init__": __init__, "__doc__": cls.__doc__})


# Tucker-factorised and spherical variants (tfno.py:619-624): their weights live in tltorch / torch_harmonics containers
# that this image does not have, so the constructors raise (SpectralConv refuses the factorization; SFNO needs the SHT).
TFNO = _with_defaults('TFNO', FNO, factorization='Tucker')
TFNO1d = _with_defaults('TFNO1d', FNO1d, factorization='Tucker')
TFNO2d = _with_defaults('TFNO2d', FNO2d, factorization='Tucker')
TFNO3d = _with_defaults('TFNO3d', FNO3d, factorization='Tucker')


class SFNO(FNO):
    def __init__(self, *args, **kwargs):
        _unsupported("SFNO (spherical harmonic convolution, torch_harmonics)")
