"""LpLoss and H1Loss with the reference surface (neuralop/training/losses.py:62-277): the same constructors, attributes
(`d`, `p`, `L`, `reduce_dims`, `reductions`, `fix_{x,y,z}_bnd`) and methods (`uniform_h`, `reduce_all`, `abs`, `rel`,
`__call__`).  The norms, their float64 sums and the gradient run in the HIP engine (functional.sobolev_loss,
csrc/k_sobolev_loss.h); there is no CPU path.

The default reduction (`reduce_dims=0`: over the batch axis of a (B, C, grid) input) happens inside the engine's finishing
kernel and no torch arithmetic runs at all; any other `reduce_dims` / `reductions` takes the engine's per-plane tensor and
applies the reference's own `reduce_all(...).squeeze()` to that small tensor.  What the engine has no kernel for raises
NotImplementedError naming the option: `p != 2`, `H1Loss.compute_terms` (the derivative fields are never materialised) and
`DissipativeLoss`.  Two stated deviations, as for functional.darcy_loss: a plane with x == y exactly gets a zero gradient
(the reference's autograd gives NaN), and `y` is data - a `y` that requires grad is refused."""
import math

import torch

from ... import functional as F


class _EngineLoss(object):
    """what LpLoss and H1Loss share: the reduction settings, the mesh width and the call into the engine"""

    def _settings(self, d, L, reduce_dims, reductions):
        self.d = d
        self.reduce_dims = [reduce_dims] if isinstance(reduce_dims, int) else reduce_dims
        if self.reduce_dims is not None:
            if isinstance(reductions, str):
                assert reductions in ("sum", "mean")
                self.reductions = [reductions] * len(self.reduce_dims)
            else:
                assert all(r in ("sum", "mean") for r in reductions)
                self.reductions = reductions
        self.L = [L] * self.d if isinstance(L, float) else L

    def uniform_h(self, x):
        """L_k / n_k on the trailing d axes, L taken right-aligned"""
        return [self.L[-j] / x.size(-j) for j in range(self.d, 0, -1)]

    def reduce_all(self, x):
        for dim, how in zip(self.reduce_dims, self.reductions):
            x = torch.sum(x, dim=dim, keepdim=True) if how == "sum" else torch.mean(x, dim=dim, keepdim=True)
        return x

    def _mesh(self, x, h):
        if h is None:
            return self.uniform_h(x)
        return [h] * self.d if isinstance(h, float) else h

    def _engine(self, x, y, h, order, relative, fix):
        if self.reduce_dims is not None and list(self.reduce_dims) == [0] and x.dim() > self.d:
            return F.sobolev_loss(x, y, self.d, h, order, relative, fix, reduce=self.reductions[0], squeeze=True)
        planes = F.sobolev_loss(x, y, self.d, h, order, relative, fix, reduce=None)
        return planes if self.reduce_dims is None else self.reduce_all(planes).squeeze()


class LpLoss(_EngineLoss):
    """relative / absolute L2 loss per plane (losses.py:62-135); p = 2 only"""

    def __init__(self, d=1, p=2, L=2 * math.pi, reduce_dims=0, reductions="sum"):
        if p != 2:
            raise NotImplementedError(f"LpLoss: p={p} (the engine's loss is the L2 norm, p=2)")
        self.p = p
        self._settings(d, L, reduce_dims, reductions)

    def abs(self, x, y, h=None):
        return self._engine(x, y, self._mesh(x, h), 0, False, (False,) * self.d)

    def rel(self, x, y):
        return self._engine(x, y, self.uniform_h(x), 0, True, (False,) * self.d)

    def __call__(self, x, y):
        return self.rel(x, y)


class H1Loss(_EngineLoss):
    """relative / absolute H1 loss per plane with central differences, periodic or one-sided at fixed ends
    (losses.py:138-277)"""

    def __init__(self, d=1, L=2 * math.pi, reduce_dims=0, reductions="sum", fix_x_bnd=False, fix_y_bnd=False, fix_z_bnd=False):
        assert d > 0 and d < 4, "Currently only implemented for 1, 2, and 3-D."
        self.fix_x_bnd, self.fix_y_bnd, self.fix_z_bnd = fix_x_bnd, fix_y_bnd, fix_z_bnd
        self._settings(d, L, reduce_dims, reductions)

    def compute_terms(self, x, y, h):
        raise NotImplementedError("H1Loss: compute_terms (the engine never materialises the derivative fields; `abs` and `rel` "
                                  "return the norms)")

    def _fix(self):
        return (bool(self.fix_x_bnd), bool(self.fix_y_bnd), bool(self.fix_z_bnd))[:self.d]

    def abs(self, x, y, h=None):
        return self._engine(x, y, self._mesh(x, h), 1, False, self._fix())

    def rel(self, x, y, h=None):
        return self._engine(x, y, self._mesh(x, h), 1, True, self._fix())

    def __call__(self, x, y, h=None):
        return self.rel(x, y, h=h)


class DissipativeLoss(object):
    """losses.py:280-324: its `__call__` reads names that nothing defines, so there is no behaviour to carry over"""

    def __init__(self, *args, **kwargs):
        raise NotImplementedError("DissipativeLoss is not part of the MI355X engine (the reference's __call__ reads undefined names)")
