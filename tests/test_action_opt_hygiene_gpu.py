"""Poisoned-buffer and guard-band cases for the entry points of the optimal-observer policy (tests/hygiene.py): outputs and
the workspace pre-filled with 0x00 / 0xFF (NaN) / 0x7F patterns inside guard bands, inputs inside NaN-filled guarded buffers.
Every output is bitwise equal across the runs and finite, the guard bands are intact, the inputs come back unchanged; the
operands an entry point updates in place (the action, its Adam moments, the observer input) are allocated inside the case, so
they are poisoned too.

Safety (hygiene.py's rule: poison only data): the kernels of k_action_opt.h read and write planes of floats and doubles, the
objective's workspace holds partial sums, k_lift_dx reads a gradient and a weight matrix.  Nothing a kernel turns into an
address lives in a poisoned buffer."""
import math

import pytest
import torch

from tests import action_opt_cases as A
from tests import hygiene as H
from tests.judging import dev  # noqa: F401

pytestmark = pytest.mark.gpu
SHAPES = [(1, 1, 1), (2, 3, 257), (3, 3, 1024), (2, 2, 1020)]          # (B, P, plane)


def _inputs(dev, B, P, plane):
    g = torch.Generator().manual_seed(1000 * B + 10 * P + plane)
    r = lambda *s, dt=torch.float32: torch.randn(*s, generator=g, dtype=dt).to(dev)      # noqa: E731
    return {"v0": 0.3 * r(B, plane, 1, dt=torch.float64), "mean": 0.05 * r(plane, dt=torch.float64),
            "std": 0.2 + 0.1 * torch.rand(plane, generator=g, dtype=torch.float64).to(dev), "y": r(B, P, plane), "a0": 0.3 * r(B, plane),
            "dx1": 1e-3 * r(B, plane), "dx2": 1e-3 * r(B, plane)}


@pytest.mark.parametrize("B,P,plane", SHAPES)
def test_begin_and_finish(dev, B, P, plane):
    from pde_policylearning_amd import functional as F

    def fn(inp, after_forward):
        a = F.torch.empty((B, plane), dtype=torch.float32, device=dev)                 # poisoned while a pattern is active
        x = F.torch.empty((B, 3, plane), dtype=torch.float32, device=dev)
        dense = F.torch.empty((B, plane, 1, 1), dtype=torch.float32, device=dev)
        F.ctrl_action_begin(inp["v0"], inp["mean"], inp["std"], A.EPS, a, x, batch_stride=3 * plane)
        F.ctrl_action_begin(inp["v0"], inp["mean"], inp["std"], A.EPS, a, dense)
        opV2 = F.ctrl_action_finish(inp["a0"], shape=(B, plane, 1))
        after_forward()
        return {"a": a, "x channel 0": x[:, 0], "x dense": dense, "opV2": opV2}
    H.assert_clean(f"ctrl_action_begin / _finish B={B} plane={plane}", fn, _inputs(dev, B, P, plane))


@pytest.mark.parametrize("B,P,plane", SHAPES)
def test_objective(dev, B, P, plane):
    from pde_policylearning_amd import functional as F

    def fn(inp, after_forward):
        parts, dy = F.ctrl_action_objective(inp["y"], inp["a0"], inp["mean"], inp["std"], A.EPS, reg=0.1)
        after_forward()
        return {"parts": parts, "dy": dy}
    H.assert_clean(f"ctrl_action_objective B={B} P={P} plane={plane}", fn, _inputs(dev, B, P, plane))


@pytest.mark.parametrize("B,P,plane", SHAPES)
def test_update(dev, B, P, plane):
    """two chained steps: the first must not read the (poisoned) moments, the second reads what the first left"""
    from pde_policylearning_amd import functional as F

    def fn(inp, after_forward):
        a, m, v = (F.torch.empty((B, plane), dtype=torch.float32, device=dev) for _ in range(3))
        x = F.torch.empty((B, 3, plane), dtype=torch.float32, device=dev)
        a.copy_(inp["a0"])
        for step, dx in ((1, inp["dx1"]), (2, inp["dx2"])):
            parts = torch.zeros((B, 3), dtype=torch.float64, device=dev)
            parts[:, 2] = a.double().norm(dim=1)
            F.ctrl_action_update(dx, parts, inp["mean"], inp["std"], A.EPS, a, m, v, x, step, reg=0.1, batch_stride=3 * plane)
        after_forward()
        return {"a": a, "exp_avg": m, "exp_avg_sq": v, "x channel 0": x[:, 0]}
    H.assert_clean(f"ctrl_action_update B={B} plane={plane}", fn, _inputs(dev, B, P, plane))


@pytest.mark.parametrize("B,cin,C,plane", [(1, 1, 64, 1024), (2, 4, 32, 128), (3, 1, 32, 3072)])
def test_lifting_input_gradient(dev, B, cin, C, plane):
    from pde_policylearning_amd import functional as F
    g = torch.Generator().manual_seed(B + cin + C + plane)
    r = lambda *s: torch.randn(*s, generator=g).to(dev)      # noqa: E731
    inputs = {"x": r(B, cin, plane // 32, 32).requires_grad_(True), "w": (r(C, cin) / math.sqrt(cin)).requires_grad_(True),
              "b": r(C).requires_grad_(True), "dy": r(B, C, plane // 32, 32)}

    def fn(inp, after_forward):
        y = F.lifting(inp["x"], inp["w"], inp["b"])
        after_forward()
        dx, dw, db = torch.autograd.grad(y, (inp["x"], inp["w"], inp["b"]), inp["dy"])
        return {"y": y, "dx": dx, "dw": dw, "db": db}
    H.assert_clean(f"lifting with dx B={B} cin={cin} C={C} plane={plane}", fn, inputs)
