"""Memory hygiene of functional.data_transpose_gather and functional.pino_input (tests/hygiene.py): the same bits with plain
allocations and with every buffer the wrappers allocate poisoned (0x00, 0xFF, 0x7F) inside guard bands, the guard bands intact,
the pool and the axis vectors unchanged.  The kernels own every element of a new output - the scalar heads and tails around the
16-byte quads of every column block included - so one they forgot would keep the poison and differ between the runs; a store
past the output's end lands in a guard band, and so does a read past the pool's (NaN there: it would show in the result).
Neither kernel has a workspace.  The one buffer whose content becomes an address, the uploaded index vector, is not allocated
through torch.empty / _bytes (`idx.to(device)` of the host-checked indices), so the harness never poisons it."""
import pytest
import torch

from tests import hygiene as H
from tests import pino_device_data_cases as K
from tests.judging import dev  # noqa: F401

pytestmark = pytest.mark.gpu

IDX = torch.tensor([4, 0, 3, 3, 5])


@pytest.mark.parametrize("rows, cols", [(7, 225), (65, 1024), (129, 256)], ids=["7x225", "65x1024", "129x256"])
def test_transpose_gather(dev, rows, cols):  # noqa: F811
    from pde_policylearning_amd import _lib
    from pde_policylearning_amd import functional as F
    host = K.pool((K.N_SRC, rows, cols), 31)

    def fn(inp, after_forward):
        with _lib.launch_log() as log:
            out = F.data_transpose_gather(inp["pool"], IDX)
        K.assert_launched(log, [K.transpose_launch(rows, cols, 5)])
        after_forward()
        return {"out": out}
    out = H.assert_clean(f"data_transpose_gather {rows} x {cols}", fn, {"pool": host.to(dev)})["out"]
    assert K.same_bits(out.cpu(), host[IDX].transpose(1, 2)) is None


@pytest.mark.parametrize("s1, s2, t", [(3, 5, 2), (15, 15, 7), (32, 32, 65)], ids=["3x5x2", "15x15x7", "32x32x65"])
def test_pino_input(dev, s1, s2, t):  # noqa: F811
    from pde_policylearning_amd import _lib
    from pde_policylearning_amd import functional as F
    host = K.pool((K.N_SRC, s1, s2), 32)
    gh = K.axes(s1, s2, t)

    def fn(inp, after_forward):
        with _lib.launch_log() as log:
            out = F.pino_input(inp["a0"], IDX, inp["gx"], inp["gy"], inp["gt"])
        K.assert_launched(log, [K.input_launch(s1, s2, 5)])
        after_forward()
        return {"out": out}
    inputs = {"a0": host.to(dev), "gx": gh[0].to(dev), "gy": gh[1].to(dev), "gt": gh[2].to(dev)}
    out = H.assert_clean(f"pino_input {s1} x {s2} x {t}", fn, inputs)["out"]
    assert K.same_bits(out.cpu(), K.host_input(host, IDX, *gh)) is None
