"""Memory hygiene of the Darcy residual loss (tests/hygiene.py): the same bits with plain allocations and with every buffer
poisoned (0x00, 0xFF, 0x7F) inside guard bands, finite outputs, intact guard bands, unchanged inputs.  The workspace holds
float and double data only (fno_abi.hip carve_darcy: Du, the float64 partial sums, the float64 norms) - nothing in it becomes
an address."""
import pytest
import torch

from tests import darcy_cases as K
from tests import hygiene as H
from tests.judging import dev  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("shape", [(1, 5), (2, 2 * K.T + 5), (2, 61)])
def test_loss(dev, shape):  # noqa: F811
    from pde_policylearning_amd import functional as F
    t = K.make_inputs("white", shape)
    inputs = {"out": t["out"].to(dev).requires_grad_(True), "a": t["a"].to(dev), "y": t["y"].to(dev), "mol": t["mol"].to(dev)}

    def fn(inp, after_forward):
        loss_data, loss_f = F.darcy_loss(inp["out"], inp["a"], inp["y"], inp["mol"])
        alone = F.darcy_loss(inp["out"], inp["a"])
        field = F.darcy_residual(inp["out"], inp["a"], inp["mol"])
        after_forward()
        (dout,) = torch.autograd.grad(K.DATA_WEIGHT * loss_data + loss_f, [inp["out"]])
        (dalone,) = torch.autograd.grad(alone, [inp["out"]])
        return {"loss_data": loss_data, "loss_f": loss_f, "loss_f alone": alone, "field": field, "dout": dout, "dout alone": dalone}
    H.assert_clean(f"darcy_loss {shape}", fn, inputs)
