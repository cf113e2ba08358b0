"""Memory hygiene of domain padding (tests/hygiene.py): functional.domain_pad / domain_crop and a padded model give the same
bits with plain allocations and with every buffer poisoned (0x00, 0xFF, 0x7F) inside guard bands, the guard bands stay intact and
the inputs come back unchanged.  The pad kernel owns every element of its output: a margin element it forgot would keep the
poison and show up here as a difference between the runs (and, under 0xFF, as a NaN) - value tests on fresh allocations
cannot see it.  Neither kernel has a workspace, and nothing they read becomes an address."""
import pytest
import torch

from tests import domain_padding_cases as K
from tests import hygiene as H
from tests.judging import dev  # noqa: F401

pytestmark = pytest.mark.gpu

OPS = {c[0]: c for c in K.OP_CASES}


@pytest.mark.parametrize("name", ["2 nothing aligned", "2 symmetric", "6 3-D symmetric", "9 pads larger than the interior"])
def test_op(dev, name):  # noqa: F811
    from pde_policylearning_amd import functional as F
    _, shape, before, after = OPS[name]
    x = K.op_input(name, shape, specials=False)           # (the harness requires finite outputs)
    y = K.pad(x, before, after)
    inputs = {"x": x.to(dev).requires_grad_(True), "gy": K.op_input(name + ".gy", tuple(y.shape), specials=False).to(dev),
              "y": K.op_input(name + ".y", tuple(y.shape), specials=False).to(dev).requires_grad_(True),
              "gx": K.op_input(name + ".gx", shape, specials=False).to(dev)}

    def fn(inp, after_forward):
        p = F.domain_pad(inp["x"], before, after)
        c = F.domain_crop(inp["y"], before, after)
        after_forward()
        dx, = torch.autograd.grad(p, inp["x"], inp["gy"])
        dy, = torch.autograd.grad(c, inp["y"], inp["gx"])
        return {"pad": p, "crop": c, "pad backward": dx, "crop backward": dy}
    out = H.assert_clean(f"domain_pad / domain_crop {name}", fn, inputs)
    assert torch.equal(K.bits(out["pad"]), K.bits(y)) and torch.equal(K.bits(out["crop backward"]), K.bits(K.pad(inputs["gx"].cpu(), before, after)))


def test_model(dev):  # noqa: F811
    cname = "tiled"
    p, x = K.model_params(cname)
    model = K.load_model(cname, p, dev)
    names = [n for n, _ in model.named_parameters()]

    def fn(inp, after_forward):
        y = torch.func.functional_call(model, {n: inp[n] for n in names}, (inp["x"],))
        after_forward()
        grads = torch.autograd.grad(y.square().sum(), [inp[n] for n in names])
        return {"y": y, **{"grad " + n: g for n, g in zip(names, grads)}}
    inputs = {n: prm.detach().clone().requires_grad_(True) for n, prm in model.named_parameters()}
    inputs["x"] = x.to(dev)
    H.assert_clean(f"model {cname} with domain padding", fn, inputs)
