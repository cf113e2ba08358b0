"""Poisoned-buffer and guard-band cases for the entry points of the optimal-policy-observer policy (tests/hygiene.py): outputs
pre-filled with 0x00 / 0xFF (NaN) / 0x7F patterns inside guard bands, inputs inside NaN-filled guarded buffers.  Every output
is bitwise equal across the runs and finite, the guard bands are intact, the inputs come back unchanged.

Safety (hygiene.py's rule: poison only data): the kernels of k_policy_opt.h read and write planes of floats and doubles and
the (B, 3) loss parts; nothing a kernel turns into an address lives in a poisoned buffer."""
import pytest
import torch

from tests import hygiene as H
from tests.judging import dev  # noqa: F401

pytestmark = pytest.mark.gpu
SHAPES = [(1, 1), (3, 1), (2, 1020), (3, 1020)]          # (B, plane)


def _inputs(dev, B, plane):
    g = torch.Generator().manual_seed(1000 * B + plane)
    r = lambda *s, dt=torch.float32: torch.randn(*s, generator=g, dtype=dt).to(dev)      # noqa: E731
    x = 0.3 * r(B, plane)
    parts = torch.zeros(B, 3, dtype=torch.float64, device=dev)
    parts[:, 2] = x.double().norm(dim=1)
    return {"v0": 0.3 * r(B, plane, 1, dt=torch.float64), "p2": 2.0 * r(B, plane, 1, dt=torch.float64), "a0": 0.3 * r(B, plane),
            "res": 0.05 * r(B, plane, 1, 1, 1), "dx": 1e-3 * r(B, plane), "x": x, "parts": parts}


@pytest.mark.parametrize("B,plane", SHAPES)
def test_begin(dev, B, plane):
    from pde_policylearning_amd import functional as F

    def fn(inp, after_forward):
        a0 = F.torch.empty((B, plane), dtype=torch.float32, device=dev)                 # poisoned while a pattern is active
        pin = F.torch.empty((B, plane, 1, 1, 1), dtype=torch.float32, device=dev)
        F.ctrl_policy_begin(inp["v0"], inp["p2"], a0, pin)
        after_forward()
        return {"a0": a0, "pin": pin}
    H.assert_clean(f"ctrl_policy_begin B={B} plane={plane}", fn, _inputs(dev, B, plane))


@pytest.mark.parametrize("B,plane", SHAPES)
def test_compose(dev, B, plane):
    from pde_policylearning_amd import functional as F

    def fn(inp, after_forward):
        x = F.torch.empty((B, plane, 1, 1, 1), dtype=torch.float32, device=dev)
        opV2 = F.torch.empty((B, plane, 1), dtype=torch.float64, device=dev)
        F.ctrl_policy_compose(inp["a0"], inp["res"], x, opV2)
        after_forward()
        return {"x": x, "opV2": opV2}
    H.assert_clean(f"ctrl_policy_compose B={B} plane={plane}", fn, _inputs(dev, B, plane))


@pytest.mark.parametrize("B,plane", SHAPES)
def test_grad(dev, B, plane):
    from pde_policylearning_amd import functional as F

    def fn(inp, after_forward):
        g = F.ctrl_policy_grad(inp["dx"], inp["x"], inp["parts"], reg=0.1)
        given = F.torch.empty((B, plane), dtype=torch.float32, device=dev)
        F.ctrl_policy_grad(inp["dx"], inp["x"], inp["parts"], reg=0.0, out=given)
        after_forward()
        return {"g": g, "g at reg 0": given}
    H.assert_clean(f"ctrl_policy_grad B={B} plane={plane}", fn, _inputs(dev, B, plane))
