"""What the entry scripts take from `from libs.utilities3 import *` (run_pde_observers.py:9, run_control.py:10), with the
reference surface:
  NormalizerGivenMeanStd (libs/utilities3.py:76-132): pointwise Gaussian normalisation with given statistics.  The device
      copies are made lazily (the reference calls `.cuda()` in the constructor); `cuda_decode` is what trainer.FusedLpLoss
      fuses into the loss kernels.
  LpLoss (:295-337): trainer.LpLoss, re-exported.
  HsLoss (:339-405): the spectral Sobolev loss, on the engine (functional.hs_loss, csrc/k_hs_loss.h).
  count_params (:438-443).
The other classes of the file (UnitGaussianNormalizer, GaussianNormalizer, RangeNormalizer*, MatReader, DenseNet) are read by
nothing on the accelerated paths and are not here."""
import numpy as np
import torch

from ..trainer import LpLoss  # noqa: F401  (re-exported: the star import carries it, as it carries np and torch)


class NormalizerGivenMeanStd(object):
    def __init__(self, mean, std, plane_indexs=None, eps=0.00001, time_last=True):
        if plane_indexs is not None:
            mean = mean[:, plane_indexs, :]
            std = std[:, plane_indexs, :]
        if np.sum(abs(np.asarray(mean) - eps)) < eps:
            raise RuntimeError("Provided mean is zero!")
        self.mean = torch.as_tensor(np.asarray(mean))
        self.std = torch.as_tensor(np.asarray(std))
        self.eps = eps
        self.time_last = time_last
        self._dev = {}

    def _on(self, device):
        key = str(device)
        if key not in self._dev:
            self._dev[key] = (self.mean.to(device), self.std.to(device))
        return self._dev[key]

    @property
    def mean_cuda(self):
        return self._on("cuda")[0]

    @property
    def std_cuda(self):
        return self._on("cuda")[1]

    def encode(self, x):
        return (x - self.mean) / (self.std + self.eps)

    def cuda_encode(self, x):
        mean, std = self._on(x.device)
        return (x - mean) / (std + self.eps)

    def decode(self, x, sample_idx=None):
        if sample_idx is not None:
            raise NotImplementedError("sample_idx masks are outside the observer training path")
        return x * (self.std + self.eps) + self.mean

    def cuda_decode(self, x, sample_idx=None):
        if sample_idx is not None:
            raise NotImplementedError("sample_idx masks are outside the observer training path")
        mean, std = self._on(x.device)
        return x * (std + self.eps) + mean


class HsLoss(object):
    """Sobolev (Hs) norm in Fourier space, libs/utilities3.py:339-405: constructor, attributes, `rel` and `__call__` of the
    reference; `__call__` runs in the engine (forward two launches, backward one), on x, y (B, N, N, *rest) float32 on the GPU
    with N = 32, 64 or 128.  Deviations: p != 2 raises (the reference takes any p into torch.norm); k = 0 with group=False
    raises ValueError (the reference dies there inside torch.sqrt of an int); y is data; a sample with x == y gets a zero
    gradient (the reference: NaN).  As the reference, `d` is stored and unused and `__call__` ignores its `a`."""

    def __init__(self, d=2, p=2, k=1, a=None, group=False, size_average=True, reduction=True):
        assert d > 0 and p > 0
        if p != 2:
            raise NotImplementedError(f"HsLoss: p={p} (the engine's kernels sum squares: p = 2)")
        if k == 0 and not group:
            raise ValueError("HsLoss: k=0 with group=False (the reference fails there: torch.sqrt of the int weight 1); "
                             "LpLoss is that loss")
        self.d, self.p, self.k, self.balanced = d, p, k, group
        self.reduction, self.size_average = reduction, size_average
        self.a = [1] * k if a is None else a      # one coefficient per derivative order; `group` is kept as `balanced`

    rel = LpLoss.rel      # the plain relative L2 of the physical fields: the same arithmetic on p, reduction, size_average

    def __call__(self, x, y, a=None):
        from .. import functional as F
        reduce = ("mean" if self.size_average else "sum") if self.reduction else None
        return F.hs_loss(x, y, k=self.k, a=self.a, group=bool(self.balanced), reduce=reduce)


def count_params(model):
    return sum(p.numel() * (2 if p.is_complex() else 1) for p in model.parameters())
