"""Memory hygiene of the one-dimensional spectral convolution (tests/hygiene.py): the same bits with plain allocations and with
every buffer poisoned (0x00, 0xFF, 0x7F) inside guard bands, finite outputs, intact guard bands, unchanged inputs.  The 1-D
workspace and the buffer saved for the backward hold float data only (fno_abi.hip carve_spec1d): slab partial spectra, the
mixed spectrum, slab sums of dy, the input spectrum and a packed copy of the weights - nothing in them becomes an address."""
import pytest
import torch

from tests import fno1d_cases as K
from tests import hygiene as H
from tests.judging import dev  # noqa: F401

pytestmark = pytest.mark.gpu


def _real(t):
    """the complex weight as the real (.., 2) tensor the engine reads (the harness poisons and compares real buffers)"""
    return torch.view_as_real(t).contiguous() if t.is_complex() else t


@pytest.mark.parametrize("name", ["A_one_tile", "C_three_tiles"])
def test_conv(dev, name):  # noqa: F811
    from pde_policylearning_amd import functional as F
    case, t = K.CASE[name], K.inputs(name)
    inputs = {k: _real(v).to(dev).requires_grad_(k != "dy") for k, v in t.items() if v is not None}

    def fn(inp, after_forward):
        y = F.spectral_conv(inp["x"], [inp["w"]], inp.get("bias"), (case.M,), case.norm)
        after_forward()
        names = [k for k in ("x", "w", "bias") if k in inp]
        grads = torch.autograd.grad(y, [inp[k] for k in names], inp["dy"])
        return {"y": y, **{"d" + k: g for k, g in zip(names, grads)}}
    H.assert_clean(f"spectral_conv 1-D {name}", fn, inputs)


@pytest.mark.parametrize("gelu", [False, True])
def test_layer(dev, gelu):  # noqa: F811
    from pde_policylearning_amd import functional as F
    case, t = K.LAYER, K.inputs(K.LAYER.name)
    inputs = {k: _real(v).to(dev).requires_grad_(k != "dy") for k, v in t.items()}

    def fn(inp, after_forward):
        y = F.spectral_pointwise_layer(inp["x"], [inp["w"]], (case.M,), case.norm, inp["pw"], inp["bias"], input_gelu=gelu)
        after_forward()
        names = ("x", "w", "pw", "bias")
        grads = torch.autograd.grad(y, [inp[k] for k in names], inp["dy"])
        return {"y": y, **{"d" + k: g for k, g in zip(names, grads)}}
    H.assert_clean(f"spectral_pointwise_layer 1-D input_gelu={int(gelu)}", fn, inputs)


def test_model(dev):  # noqa: F811
    from pde_policylearning_amd.neuralop.models import FNO1d
    model = FNO1d(16, 32, in_channels=2, out_channels=1).to(dev)
    p = K.neuralop_params(model, "nop.hygiene")
    names = list(p)

    def fn(inp, after_forward):
        y = torch.func.functional_call(model, {n: inp[n] for n in names}, (inp["x"],))
        after_forward()
        grads = torch.autograd.grad(y.square().sum(), [inp[n] for n in names])
        return {"y": y, **{"grad " + n: g for n, g in zip(names, grads)}}
    inputs = {n: v.to(dev).requires_grad_(True) for n, v in p.items()}
    inputs["x"] = K._t("nop.hygiene.x", (2, 2, 256), 1.0).to(dev)
    H.assert_clean("neuralop FNO1d", fn, inputs)
