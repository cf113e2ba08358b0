"""Memory hygiene of the Sobolev / L2 training losses (tests/hygiene.py): the same bits with plain allocations and with every
buffer poisoned (0x00, 0xFF, 0x7F) inside guard bands, finite outputs, intact guard bands, unchanged inputs.  The workspace
holds float and double data only (fno_abi.hip carve_sobolev: the float64 partial sums of every workgroup and the float64
(num, den) of every plane; the values are a float tensor of their own) - nothing in it becomes an address."""
import pytest
import torch

from tests import hygiene as H
from tests import sobolev_cases as K
from tests.judging import dev  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("shape,d", [((2, 3, 2), 1), ((2, 1, K.T2[0] + 1, K.T2[1] + 1), 2), ((2, 3, 61, 61), 2)],
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else f"d{v}")
def test_loss(dev, shape, d):  # noqa: F811
    """forward and backward of H1 with fixed boundaries (fused reduction and per plane) and of Lp"""
    from pde_policylearning_amd.neuralop.training import H1Loss, LpLoss
    x, y = K.make_inputs("white", shape, d)
    inputs = {"x": x.to(dev).requires_grad_(True), "y": y.to(dev)}
    flags = dict(zip(("fix_x_bnd", "fix_y_bnd", "fix_z_bnd"), (True,) * d))
    h1, h1_planes, lp = H1Loss(d=d, **flags), H1Loss(d=d, reduce_dims=None, reductions="mean", **flags), LpLoss(d=d, reductions="mean")

    def fn(inp, after_forward):
        a, b, c = h1(inp["x"], inp["y"]), h1_planes.abs(inp["x"], inp["y"]), lp(inp["x"], inp["y"])
        after_forward()
        (da,) = torch.autograd.grad(a.sum(), [inp["x"]])
        (db,) = torch.autograd.grad(b.sum(), [inp["x"]])
        (dc,) = torch.autograd.grad(c.sum(), [inp["x"]])
        return {"h1 rel": a, "h1 abs planes": b, "lp rel": c, "dx h1 rel": da, "dx h1 abs": db, "dx lp": dc}
    H.assert_clean(f"sobolev_loss {shape}", fn, inputs)
