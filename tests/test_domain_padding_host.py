"""Domain padding, the part that needs no GPU: the restatement of tests/domain_padding_cases.py against the reference's recorded
tensors (bit for bit), the grids on which the reference does not round-trip, the constructor surface, pickles, every refusal,
and the C ABI's argument checks."""
import ctypes
import io
import pickle

import numpy as np
import pytest
import torch

from tests import domain_padding_cases as K


@pytest.fixture(scope="module")
def lib():
    from pde_policylearning_amd import build, _lib
    build.build()
    return _lib.lib()


@pytest.fixture(scope="module")
def golden():
    return np.load(K.GOLDEN)


def test_golden_file_holds_the_listed_cases_and_nothing_else(golden):
    want = {K.golden_key(g, f, m) + "/" + part for g, f in K.GOLDEN_GRIDS for m in K.MODES for part in ("x", "padded", "unpadded")}
    assert set(golden.files) == want


@pytest.mark.parametrize("mode", K.MODES)
@pytest.mark.parametrize("grid, frac", K.GOLDEN_GRIDS)
def test_restatement_equals_the_reference_bitwise(golden, grid, frac, mode):
    """pad and unpad of tests/domain_padding_cases.py and the amounts of DomainPadding against what the reference's own
    DomainPadding produced on the grids where it round-trips, as int32 images (NaN, both infinities and -0.0 are in the input)"""
    from pde_policylearning_amd.neuralop.models import DomainPadding
    key = K.golden_key(grid, frac, mode)
    x = torch.from_numpy(golden[key + "/x"])
    assert torch.equal(K.bits(x), K.bits(K.golden_input(grid)))
    before, after = K.amounts(grid, frac, mode)
    y = K.pad(x, before, after)
    assert tuple(y.shape[2:]) == K.GOLDEN_PADDED[(mode, grid)] == tuple(golden[key + "/padded"].shape[2:])
    assert torch.equal(K.bits(y), K.bits(torch.from_numpy(golden[key + "/padded"])))
    z = K.unpad(y, before, after)
    assert torch.equal(K.bits(z), K.bits(torch.from_numpy(golden[key + "/unpadded"]))) and torch.equal(K.bits(z), K.bits(x))
    # every margin element is +0.0
    margin = torch.ones(y.shape, dtype=torch.bool)
    margin[(Ellipsis,) + tuple(slice(b, b + r) for b, r in zip(before, grid))] = False
    assert int(K.bits(y)[margin].abs().max()) == 0
    dp = DomainPadding(frac, mode.upper())
    assert dp.amounts(grid) == (before, after) and dp.padded_resolution(grid) == K.GOLDEN_PADDED[(mode, grid)]


@pytest.mark.parametrize("grid, frac, padded", K.NON_SQUARE)
def test_grids_with_unequal_amounts_round_trip(grid, frac, padded):
    """(32, 64), (8, 8, 12) and (2, 40) at 0.25: the reference pads to (48, 72) / (11, 10, 14) / - and unpads to (40, 56) /
    (9, 8, 11) / an empty tensor; here axis d gets its own round(f * r_d) both ways and an amount of 0 leaves the axis alone"""
    from pde_policylearning_amd.neuralop.models import DomainPadding
    before, after = K.amounts(grid, frac, "one-sided")
    assert before == (0,) * len(grid) and after == tuple(int(round(frac * r)) for r in grid)
    x = K.golden_input(grid)
    y = K.pad(x, before, after)
    assert tuple(y.shape[2:]) == padded
    assert torch.equal(K.bits(K.unpad(y, before, after)), K.bits(x))
    assert torch.equal(K.bits(y[(Ellipsis,) + tuple(slice(0, r) for r in grid)]), K.bits(x))      # the interior sits at index 0
    dp = DomainPadding(frac)
    assert dp.amounts(grid) == (before, after) and dp.padded_resolution(grid) == padded
    sym = DomainPadding(frac, "symmetric")
    assert sym.amounts(grid) == (after, after)
    assert DomainPadding([0.5, 0.25]).amounts((32, 64)) == ((0, 0), (16, 16))


def test_constructor_surface():
    from pde_policylearning_amd.neuralop.models import FNO, FNO1d, FNO2d, FNO3d, DomainPadding
    plain = FNO2d(8, 8, 32)
    for m in (plain, FNO2d(8, 8, 32, domain_padding=None), FNO2d(8, 8, 32, domain_padding=0), FNO2d(8, 8, 32, domain_padding=0.0)):
        assert m.domain_padding is None and m.domain_padding_mode == "one-sided"
        assert list(m.state_dict()) == list(plain.state_dict())
        assert "domain_padding" not in dict(m.named_children())
    m = FNO2d(8, 8, 32, domain_padding=0.25, domain_padding_mode="Symmetric")
    assert isinstance(m.domain_padding, DomainPadding) and m.domain_padding_mode == "Symmetric"
    assert m.domain_padding.padding_mode == "symmetric" and m.domain_padding.domain_padding == 0.25
    assert m.domain_padding.output_scaling_factor is None
    assert list(m.state_dict()) == list(plain.state_dict())                    # the padding has no parameters or buffers
    for cls, pos in ((FNO, ((8, 8), 32)), (FNO3d, (8, 8, 8, 32)), (FNO1d, (16, 32))):
        assert isinstance(cls(*pos, domain_padding=0.5).domain_padding, DomainPadding)
        assert cls(*pos).domain_padding is None
    with pytest.raises(ValueError, match="padding_mode"):
        FNO2d(8, 8, 32, domain_padding=0.25, domain_padding_mode="reflect")
    with pytest.raises(ValueError, match="padding_mode"):
        DomainPadding(0.25, "circular")
    with pytest.raises(NotImplementedError, match="output_scaling_factor"):
        FNO((8, 8), 32, domain_padding=0.25, output_scaling_factor=2)
    with pytest.raises(NotImplementedError, match="output_scaling_factor"):
        DomainPadding(0.25, output_scaling_factor=2)
    # FNO1d keeps its own refusals with the option on
    for kw in (dict(use_mlp=True), dict(separable=True), dict(output_scaling_factor=2), dict(norm="group_norm"), dict(preactivation=True)):
        with pytest.raises(NotImplementedError):
            FNO1d(16, 32, domain_padding=0.5, **kw)


def test_fused_supported_is_off_with_padding_and_unchanged_without():
    """fused_supported answers False before it looks at the tensor when padding is on; without it the answer is what it was
    (a CPU tensor is refused by the shape rule, not by the new test)"""
    from pde_policylearning_amd.neuralop.models import FNO2d
    x = torch.zeros(2, 3, 64, 64)
    assert FNO2d(8, 8, 32, domain_padding=0.25).fused_supported(x) is False
    assert not FNO2d(8, 8, 32).fused_supported(x) and not FNO2d(8, 8, 32, domain_padding=0).fused_supported(x)


def test_get_model_passes_the_option_through():
    from pde_policylearning_amd.neuralop.models import DomainPadding, FNO2d, get_model
    cfg = {"arch": "fno2d",
           "fno2d": dict(data_channels=3, n_modes_height=8, n_modes_width=8, hidden_channels=32, n_layers=4, domain_padding=0.25,
                         domain_padding_mode='symmetric', fft_norm='forward'),
           "patching": {"levels": 0}}
    m = get_model(cfg)
    assert type(m) is FNO2d and isinstance(m.domain_padding, DomainPadding)
    assert m.domain_padding.padding_mode == "symmetric" and m.domain_padding.amounts((32, 32)) == ((8, 8), (8, 8))


def test_pickle_round_trip_and_modules_pickled_before_the_option():
    from pde_policylearning_amd.neuralop.models import FNO1d, FNO2d
    m = FNO2d(8, 8, 32, domain_padding=0.25)
    m.domain_padding.amounts((32, 32))              # a model that has seen a resolution carries its cache along
    buf = io.BytesIO()
    pickle.dump(m, buf)
    m2 = pickle.loads(buf.getvalue())
    sd, sd2 = m.state_dict(), m2.state_dict()
    assert type(m2) is type(m) and list(sd) == list(sd2) and all(torch.equal(sd[k], sd2[k]) for k in sd)
    assert m2.domain_padding.amounts((32, 32)) == ((0, 0), (8, 8)) and m2.domain_padding_mode == "one-sided"
    # a module pickled before the option existed has neither attribute
    for old in (FNO2d(8, 8, 32), FNO1d(16, 32)):
        for name in ("domain_padding", "domain_padding_mode"):
            del old.__dict__[name]
        assert not hasattr(old, "domain_padding")
        assert old.fused_supported(torch.zeros(2, 3, 64, 64)) is False        # (a CPU tensor: refused by the shape rule)
        with pytest.raises(RuntimeError, match="GPU"):                         # forward() gets as far as the device check
            old(torch.zeros(2, 3, 128) if isinstance(old, FNO1d) else torch.zeros(2, 3, 64, 64))


def test_cpu_and_wrong_dtype_tensors_are_refused():
    from pde_policylearning_amd import functional as F
    from pde_policylearning_amd.neuralop.models import DomainPadding, FNO1d, FNO2d
    x = torch.zeros(2, 3, 5, 7)
    for fn in (F.domain_pad, F.domain_crop):
        with pytest.raises(RuntimeError, match="GPU"):
            fn(x, (0, 0), (1, 1))
    with pytest.raises(RuntimeError, match="GPU"):
        DomainPadding(0.25).pad(x)
    with pytest.raises(RuntimeError, match="GPU"):
        FNO2d(8, 8, 32, domain_padding=0.25)(torch.zeros(2, 3, 32, 32))
    with pytest.raises(RuntimeError, match="GPU"):
        FNO1d(16, 32, domain_padding=0.5)(torch.zeros(2, 3, 256))
    with pytest.raises(RuntimeError, match="no pad"):
        DomainPadding(0.25).unpad(x)
    # the dtype and shape rules sit behind the device check: driven with a stand-in that claims to be on the GPU
    with pytest.raises(RuntimeError, match="float32"):
        F._domain_operand("domain_pad", "x", _FakeCuda(torch.float64, (2, 3, 5)))
    with pytest.raises(RuntimeError, match=r"d1\[, d2\[, d3\]\]"):
        F._domain_operand("domain_pad", "x", _FakeCuda(torch.float32, (2, 3)))
    for bad in ((1,), (1, -1), (1, 1, 1)):
        with pytest.raises(RuntimeError, match="non-negative"):
            F._domain_amounts("domain_pad", 2, bad, (0, 0))


class _FakeCuda(object):
    """what _require_cuda and the shape rule read of a tensor: lets the CPU suite reach the checks behind the device check"""

    def __init__(self, dtype, shape):
        self.is_cuda, self.dtype, self.shape, self.device = True, dtype, torch.Size(shape), "cuda:0"

    def dim(self):
        return len(self.shape)


def test_abi_refuses_bad_arguments_without_a_launch(lib):
    """null pointers, ndim outside 1..3, a dimension below 1, a negative pad: FNO_EINVAL; a tensor the index arithmetic cannot
    address: FNO_EUNSUPPORTED naming the limit; nothing is launched (this machine has no GPU: a launch would be a HIP error,
    code FNO_EHIP, or a crash on the fake addresses).  All pads zero and zero planes are legal."""
    from pde_policylearning_amd import _lib
    EINVAL, EUNSUPPORTED = _lib.ABI.consts["FNO_EINVAL"], _lib.ABI.consts["FNO_EUNSUPPORTED"]
    assert {"fno_domain_pad", "fno_domain_crop"} <= set(_lib.EXPORTED_SYMBOLS)
    I3 = ctypes.c_int * 3
    P = ctypes.c_void_p(0x1000)      # never dereferenced: every call below must return before a launch
    ok = [2, 6, I3(5, 7), I3(0, 0), I3(2, 3), P, P, None]
    with _lib.launch_log() as log:
        for fn in (lib.fno_domain_pad, lib.fno_domain_crop):
            for i in (2, 3, 4, 5, 6):
                assert fn(*[None if j == i else a for j, a in enumerate(ok)]) == EINVAL, i
                assert b"null" in lib.fno_last_error()
            for ndim in (0, 4, -1):
                assert fn(ndim, *ok[1:]) == EINVAL and b"ndim" in lib.fno_last_error()
            for dims in (I3(0, 7), I3(5, -2)):
                assert fn(2, 6, dims, *ok[3:]) == EINVAL and b"dims" in lib.fno_last_error()
            assert fn(2, 6, ok[2], I3(0, -1), *ok[4:]) == EINVAL and b"negative" in lib.fno_last_error()
            assert fn(2, 6, ok[2], ok[3], I3(-3, 0), *ok[5:]) == EINVAL and b"negative" in lib.fno_last_error()
            assert fn(3, 6, I3(5, 7, 0), I3(0, 0, 0), I3(0, 0, 0), P, P, None) == EINVAL        # the third axis counts at ndim 3
            assert fn(2, 6, ok[2], ok[3], ok[4], ctypes.c_void_p(0x1002), P, None) == EINVAL and b"aligned" in lib.fno_last_error()
            assert fn(2, 6, I3(5, 1 << 30), I3(0, 0), I3(0, 1), P, P, None) == EUNSUPPORTED
            assert b"2^30" in lib.fno_last_error() and b"2^62" in lib.fno_last_error()
            assert fn(3, 1 << 40, I3(1 << 20, 1 << 20, 1 << 20), I3(0, 0, 0), I3(0, 0, 0), P, P, None) == EUNSUPPORTED
            assert fn(1, 1 << 63, I3(1), I3(0), I3(0), P, P, None) == EUNSUPPORTED
            assert fn(2, 0, *ok[2:]) == 0                                                      # no planes: nothing to do
    assert log.records == []
