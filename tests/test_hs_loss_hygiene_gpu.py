"""Memory hygiene of the spectral Sobolev loss (tests/hygiene.py): the same bits with plain allocations and with every buffer
poisoned (0x00, 0xFF, 0x7F) inside guard bands, finite outputs, intact guard bands, unchanged inputs.  The workspace holds
float64 data only (fno_abi.hip carve_hs: six sums of every workgroup and (num_j, den_j) of every sample; the values are a float
tensor of their own) - nothing in it becomes an address, and the sums of the terms a form does not use are written as zeros."""
import pytest
import torch

from tests import hs_loss_cases as K
from tests import hygiene as H
from tests.judging import dev  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("shape", [(2, 32, 32, 3), (1, 128, 128, 2)], ids=K.shape_id)
def test_loss(dev, shape):  # noqa: F811
    """forward and backward of an ungrouped form (the default, reduced) and a grouped one (k = 2, per sample)"""
    from pde_policylearning_amd.libs.utilities3 import HsLoss
    x, y = K.make_inputs("white", shape)
    inputs = {"x": x.to(dev).requires_grad_(True), "y": y.to(dev)}
    plain, grouped = HsLoss(), HsLoss(k=2, a=[0.5, 0.25], group=True, reduction=False)

    def fn(inp, after_forward):
        a, b = plain(inp["x"], inp["y"]), grouped(inp["x"], inp["y"])
        after_forward()
        (da,) = torch.autograd.grad(a, [inp["x"]])
        (db,) = torch.autograd.grad(b.sum(), [inp["x"]])
        return {"plain mean": a, "grouped samples": b, "dx plain": da, "dx grouped": db}
    H.assert_clean(f"hs_loss {shape}", fn, inputs)
