"""Memory hygiene of functional.data_gather (tests/hygiene.py): the same bits with plain allocations and with every buffer the
wrapper allocates poisoned (0x00, 0xFF, 0x7F) inside guard bands, the guard bands intact, the pool and the statistics unchanged.
The kernel owns every element of a new output - heads and tails around the 16-byte quads included - so one it forgot would
keep the poison and differ between the runs; a store past a plane's end lands in a guard band.  The kernel has no workspace.
The one buffer whose content becomes an address, the uploaded index vector, is not allocated through torch.empty / _bytes
(functional.data_gather: `idx.to(device)` of the host-checked indices), so the harness never poisons it."""
import pytest
import torch

from tests import device_data_cases as K
from tests import hygiene as H
from tests.judging import dev  # noqa: F401

pytestmark = pytest.mark.gpu

# name, pool dtype, statistics dtype (None: gather and cast), snapshot shape, view (offset, row_stride, col_stride, rows, cols)
CASES = [
    ("crop d2 5x7 f64 f64", torch.float64, torch.float64, (12, 20), (0, 40, 2, 5, 7)),
    ("crop d2 5x7 f32 f32", torch.float32, torch.float32, (12, 20), (0, 40, 2, 5, 7)),
    ("plane of a field f32 f64", torch.float32, torch.float64, (6, 8, 5), (35, 40, 1, 6, 5)),
    ("aligned 16x32 f64 f32", torch.float64, torch.float32, (16, 32), (0, 32, 1, 16, 32)),
    ("cast 16x32 f64", torch.float64, None, (16, 32), (0, 32, 1, 16, 32)),
    ("cast 3x1 f32", torch.float32, None, (12, 20), (7, 20, 1, 3, 1)),
    ("cast field f64", torch.float64, None, (6, 9, 5), (0, 45, 1, 6, 45)),
]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_gather(dev, case):  # noqa: F811
    from pde_policylearning_amd import functional as F
    name, ptype, stype, shape, view = case
    g = torch.Generator().manual_seed(5)
    idx = torch.tensor([6, 0, 3, 3, 5])
    inputs = {"pool": torch.randn((7,) + shape, generator=g, dtype=torch.float64).to(ptype).to(dev)}
    if stype is not None:
        inputs["mean"] = torch.randn(view[3], view[4], generator=g, dtype=torch.float64).to(stype).to(dev)
        inputs["std"] = (0.5 + torch.rand(view[3], view[4], generator=g, dtype=torch.float64)).to(stype).to(dev)

    def fn(inp, after_forward):
        out = F.data_gather(inp["pool"], idx, view, inp.get("mean"), inp.get("std"), 1e-5)
        after_forward()
        return {"out": out}
    out = H.assert_clean(f"data_gather {name}", fn, inputs)["out"]
    # and the values are the host expression's
    pool = inputs["pool"].cpu().reshape(7, -1)[idx]
    cols = [view[0] + view[1] * i + view[2] * j for i in range(view[3]) for j in range(view[4])]
    x = pool[:, cols].reshape(5, view[3], view[4])
    want = x if stype is None else (x - inputs["mean"].cpu()) / (inputs["std"].cpu() + 1e-5)
    assert torch.equal(out.cpu(), want.float())
