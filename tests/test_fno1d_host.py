"""CPU-side checks of the one-dimensional surface (no GPU): neuralop.models.FNO1d constructs with the reference's state_dict
keys, shapes and parameter count; what has no 1-D kernel still raises at construction; the PINO classes import from the
package with the reference's keys; fno_spec_plan_create refuses every 1-D limit under its own name before any HIP call."""
import ctypes

import pytest
import torch


@pytest.fixture(scope="module")
def lib():
    from pde_policylearning_amd import build, _lib
    build.build()
    return _lib.lib()


def test_neuralop_fno1d_surface():
    from pde_policylearning_amd.neuralop.models import FNO1d
    m = FNO1d(16, 32, in_channels=2)
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    want = {"lifting.fc.weight": (32, 2, 1), "lifting.fc.bias": (32,), "fno_blocks.convs.bias": (4, 32, 1),
            "projection.fc1.weight": (256, 32, 1), "projection.fc1.bias": (256,),
            "projection.fc2.weight": (1, 256, 1), "projection.fc2.bias": (1,)}
    for l in range(4):
        want[f"fno_blocks.convs.weight.{l}.tensor"] = (32, 32, 8, 2)       # n_modes // 2 complex bins as (.., 2)
        want[f"fno_blocks.fno_skips.{l}.weight"] = (32, 32, 1)
    assert shapes == want
    c, cin, cout, hid, L, half = 32, 2, 1, 256, 4, 8
    closed = (c * cin + c) + L * (c * c * half * 2 + c + c * c) + (hid * c + hid) + (cout * hid + cout)
    assert sum(p.numel() for p in m.parameters()) == closed == 78561
    assert [m.fno_blocks.gelu_after(l) for l in range(4)] == [True, True, False, False]
    assert FNO1d(16, 64, incremental_n_modes=(8,)).fno_blocks.convs.half_n_modes == [4]


def test_what_has_no_1d_kernel_raises_at_construction():
    from pde_policylearning_amd.neuralop.models import FNO1d, TFNO1d
    with pytest.raises(NotImplementedError, match=r"32, 64"):
        FNO1d(4, 8)
    with pytest.raises(NotImplementedError, match="Tucker"):
        TFNO1d(16, 32)
    for kw in ({"use_mlp": True}, {"separable": True}, {"output_scaling_factor": 2}, {"norm": "group_norm"},
               {"preactivation": True}):
        with pytest.raises(NotImplementedError):
            FNO1d(16, 32, **kw)


def test_forward_has_no_cpu_path():
    from pde_policylearning_amd.neuralop.models import FNO1d
    with pytest.raises(RuntimeError, match="GPU"):
        FNO1d(16, 32, in_channels=2)(torch.zeros(1, 2, 128))


def test_pino_1d_classes_have_the_reference_keys():
    from pde_policylearning_amd.libs.models import pino_models
    from pde_policylearning_amd.libs.models.pino_models import FNO1d, SpectralConv1d
    assert pino_models.FNO1d is FNO1d
    sc = SpectralConv1d(32, 64, 12)
    assert list(sc.state_dict()) == ["weights1"] and sc.weights1.shape == (32, 64, 12) and sc.weights1.dtype == torch.cfloat
    assert float(sc.weights1.detach().real.min()) >= 0 and float(sc.weights1.detach().real.max()) <= sc.scale      # scale * U[0, 1)
    assert sc.direct_grad_params() == [sc.weights1]
    m = FNO1d(modes=[12] * 3, width=32, act="gelu")
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    want = {"fc0.weight": (32, 2), "fc0.bias": (32,), "fc1.weight": (128, 32), "fc1.bias": (128,), "fc2.weight": (1, 128),
            "fc2.bias": (1,)}
    for i in range(3):
        want.update({f"sp_convs.{i}.weights1": (32, 32, 12), f"ws.{i}.weight": (32, 32, 1), f"ws.{i}.bias": (32,)})
    assert shapes == want
    with pytest.raises(ValueError):
        FNO1d(modes=[4], act="swish")


BAD_1D = [({"n": 96}, b"dims[0]"), ({"n": 16384}, b"dims[0]"), ({"cin": 48}, b"channels"), ({"m": 65}, b"modes[0]"),
          ({"n": 128, "m": 128 // 2 + 1}, b"modes[0]"), ({"planes": 1}, b"weight_planes")]


@pytest.mark.parametrize("change,names", BAD_1D, ids=[str(c) for c, _ in BAD_1D])
def test_plan_refuses_each_1d_limit_under_its_own_name(lib, change, names):
    from pde_policylearning_amd import _lib
    a = dict(n=256, cin=32, cout=32, m=16, planes=0)
    a.update(change)
    d = _lib.FnoSpecDesc()
    d.ndim, d.Cin, d.Cout = 1, a["cin"], a["cout"]
    d.dims[0], d.modes[0] = a["n"], a["m"]
    d.weight_last_extent, d.norm, d.weight_planes = a["m"], 1, a["planes"]
    h = ctypes.c_void_p()
    rc = lib.fno_spec_plan_create(ctypes.byref(d), ctypes.byref(h))     # refused before any HIP call: no GPU here
    msg = lib.fno_last_error()
    assert rc < 0 and names in msg and b"ndim" not in msg, msg


def test_ndim_4_is_still_refused_by_name(lib):
    from pde_policylearning_amd import _lib
    d = _lib.FnoSpecDesc()
    d.ndim, d.Cin, d.Cout = 4, 32, 32
    h = ctypes.c_void_p()
    assert lib.fno_spec_plan_create(ctypes.byref(d), ctypes.byref(h)) < 0
    assert b"ndim=4" in lib.fno_last_error() and b"1, 2 or 3" in lib.fno_last_error()      # the standalone plan names 1-D now
