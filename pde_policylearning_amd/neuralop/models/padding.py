"""DomainPadding with the reference surface (neuralop/models/padding.py:4-95): zero-pad the grid of a (B, C, d1, ..., dN) tensor
by a fraction of its resolution and crop it back, on the engine's pad / crop kernels (functional.domain_pad / domain_crop)."""
from torch import nn

from ... import functional as F

MODES = ('one-sided', 'symmetric')


class DomainPadding(nn.Module):
    """pad(x) extends axis d of the grid (r_0, ..., r_N) by p_d = int(round(f_d * r_d)) zeros - behind the interior in
    'one-sided' mode (the interior stays at index 0), p_d on both sides in 'symmetric' mode; unpad(x) removes what pad added.
    `domain_padding` is one fraction or one per axis; mode names are read case-insensitively.

    Where every p_d is the same positive number (square and cubic grids: (32, 32) at 0.25 -> (40, 40), (48, 48) at 1/3 ->
    (64, 64), (16, 16, 16) at 1.0 -> (32, 32, 32), (41, 41) at 0.1 -> (45, 45)) this is the reference's result bit for bit.

    Where the p_d differ the reference does not round-trip: its pad hands [0, p_0, 0, p_1] to torch's F.pad, which reads the
    list LAST dimension first, while its unpad slices in axis order.  (32, 64) at 0.25 pads to (48, 72) and "unpads" to
    (40, 56); (8, 8, 12) at 0.25 goes to (11, 10, 14) and comes back as (9, 8, 11); (2, 40) at 0.25 unpads to an empty tensor
    (p_0 = 0 and slice(None, -0) is empty), and the model returns a tensor of the wrong shape.  Here axis d is padded by its
    own p_d and cropped by the same amount, so the round trip is the identity - (32, 64) -> (40, 80) -> (32, 64), (8, 8, 12) ->
    (10, 10, 15), (2, 40) -> (2, 50) - and an axis whose amount rounds to 0 is left alone.

    `output_scaling_factor` (resized blocks) is refused: those blocks are torch compositions outside the engine's kernels.
    Nothing is printed (the reference prints every new resolution)."""

    def __init__(self, domain_padding, padding_mode='one-sided', output_scaling_factor=None):
        super().__init__()
        if output_scaling_factor is not None:
            raise NotImplementedError("fnoengine DomainPadding: output_scaling_factor is not supported together with domain "
                                      "padding (the resized blocks are torch compositions)")
        mode = str(padding_mode).lower()
        if mode not in MODES:
            raise ValueError(f"Got padding_mode={padding_mode!r}, expected one of {MODES}")
        self.domain_padding = domain_padding
        self.padding_mode = mode
        self.output_scaling_factor = None
        self._padding = {}            # resolution -> (before, after), one amount per axis
        self._unpad_amounts = {}      # padded resolution -> (before, after) of the pad that produced it

    def amounts(self, resolution):
        """(before, after) for a grid of this resolution"""
        resolution = tuple(int(r) for r in resolution)
        if resolution not in self._padding:
            f = self.domain_padding
            f = [float(f)] * len(resolution) if isinstance(f, (float, int)) else [float(v) for v in f]
            if len(f) != len(resolution):
                raise ValueError(f"domain_padding has {len(f)} fractions, the grid {resolution} has {len(resolution)} axes")
            p = tuple(int(round(v * r)) for v, r in zip(f, resolution))
            if min(p) < 0:
                raise ValueError(f"domain_padding={self.domain_padding!r} gives negative amounts {p} on the grid {resolution}")
            self._padding[resolution] = (p if self.padding_mode == 'symmetric' else (0,) * len(p), p)
        return self._padding[resolution]

    def padded_resolution(self, resolution):
        before, after = self.amounts(resolution)
        return tuple(int(r) + b + a for r, b, a in zip(resolution, before, after))

    def forward(self, x):
        return self.pad(x)

    def pad(self, x):
        before, after = self.amounts(x.shape[2:])
        y = F.domain_pad(x, before, after)
        self._unpad_amounts[tuple(y.shape[2:])] = (before, after)
        return y

    def unpad(self, x):
        try:
            before, after = self._unpad_amounts[tuple(x.shape[2:])]
        except KeyError:
            raise RuntimeError(f"DomainPadding.unpad: no pad() has produced the grid {tuple(x.shape[2:])}") from None
        return F.domain_crop(x, before, after)
