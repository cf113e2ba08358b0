"""Memory hygiene of the Burgers residual loss (tests/hygiene.py): the same bits with plain allocations and with every buffer
poisoned (0x00, 0xFF, 0x7F) inside guard bands, finite outputs, intact guard bands, unchanged inputs.  The workspace holds
float and double data only (fno_abi.hip carve_burgers: Du, ux, the float64 partial sums) - nothing in it becomes an address."""
import pytest
import torch

from tests import burgers_cases as K
from tests import hygiene as H
from tests.judging import dev  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("shape", [(2, 5, 32), (2, 2 * K.TJ + 3, 64), (3, 11, 128)])
def test_loss(dev, shape):  # noqa: F811
    from pde_policylearning_amd import functional as F
    t = K.make_inputs("white", shape)
    inputs = {"u": t["u"].to(dev).requires_grad_(True), "u0": t["u0"].to(dev)}

    def fn(inp, after_forward):
        loss_u, loss_f = F.burgers_loss(inp["u"], inp["u0"], 0.01)
        field = F.burgers_residual(inp["u"], 0.01)
        after_forward()
        (du,) = torch.autograd.grad(K.IC_WEIGHT * loss_u + loss_f, [inp["u"]])
        return {"loss_u": loss_u, "loss_f": loss_f, "field": field, "du": du}
    H.assert_clean(f"burgers_loss {shape}", fn, inputs)
