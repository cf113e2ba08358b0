"""Memory hygiene of the channel MLP (tests/hygiene.py): functional.channel_mlp and a model built on it give the same bits
with plain allocations and with every buffer poisoned (0x00, 0xFF, 0x7F) inside guard bands, the guard bands stay intact and the
inputs come back unchanged.  The backward's workspace holds float partial sums only (fno_abi.hip carve_cmlp), reduced by
k_reduce_jobs from a job list passed as kernel arguments: nothing in it becomes an address."""
import pytest
import torch

from tests import channel_mlp_cases as K
from tests import hygiene as H
from tests.judging import dev  # noqa: F401

pytestmark = pytest.mark.gpu

CASES = {c["name"]: c for c in K.OP_CASES}


@pytest.mark.parametrize("cname", ["three tiles per sample", "3-D expansion 1"])
@pytest.mark.parametrize("gelu_out", [False, True])
def test_op(dev, cname, gelu_out):  # noqa: F811
    from pde_policylearning_amd import functional as F
    t = K.op_inputs(CASES[cname])
    inputs = {k: v.to(dev).requires_grad_(k != "dy") for k, v in t.items()}

    def fn(inp, after_forward):
        y = F.channel_mlp(inp["u"], inp["x"], inp["w1"], inp["b1"], inp["w2"], inp["b2"], inp["gate"], gelu_out)
        after_forward()
        names = ("u", "x", "w1", "b1", "w2", "b2", "gate")
        grads = torch.autograd.grad(y, [inp[k] for k in names], inp["dy"])
        return {"y": y, **{"d" + k: g for k, g in zip(names, grads)}}
    H.assert_clean(f"channel_mlp {cname} gelu_out={int(gelu_out)}", fn, inputs)


def test_model(dev):  # noqa: F811
    cname = "fno2d_mlp_small"
    p, x, _ = K.model_params(cname)
    model = K.build_model(cname)
    sd = model.state_dict()
    model.load_state_dict({k: v.reshape(sd[k].shape) for k, v in p.items()})
    model = model.to(dev)
    names = [n for n, _ in model.named_parameters()]

    def fn(inp, after_forward):
        y = torch.func.functional_call(model, {n: inp[n] for n in names}, (inp["x"],))
        after_forward()
        grads = torch.autograd.grad(y.square().sum(), [inp[n] for n in names])
        return {"y": y, **{"grad " + n: g for n, g in zip(names, grads)}}
    inputs = {n: prm.detach().clone().requires_grad_(True) for n, prm in model.named_parameters()}
    inputs["x"] = x.to(dev)
    H.assert_clean(f"model {cname}", fn, inputs)
