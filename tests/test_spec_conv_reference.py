"""CPU self-test of the spectral-convolution comparison (tests/spec_conv_cases.py), on the cases of tests/test_spec_conv_gpu.py:
  - the float32 oracle alone stays under the floor (2e-6) on every judged quantity of every case and leaves no energy off the
    kept set, so the budget 1.75 x e_ref32 never exceeds the floor and a correct float32 kernel can meet every row;
  - the float64 oracle is exact on the structural zeros and leaks 1e-16: the kept set and the zero masks, both built from the
    mode indices, are the operator's own;
  - faults planted in a float64 copy of the oracle's results - where the fault is the only error there is - are each refused by
    the slice that looks at them.  Two of them (one kept mode of y off by 2e-5, 1e-5 of one mode leaking into a bin off the kept
    set) and the single-row fault pass the whole-tensor line of tests/test_parity_gpu.py (TOL_COMP against the float32 oracle):
    that line cannot see them.  The other three as the route table suggests them - every fourth row of a sample copied from the
    row above it, the last Ktot % 4 modes of dW summed over one sample, the last Cin % it input channels of dW missing - are
    gross where they strike (0.11, 6.4e-2 and 0.45 of the whole tensor): any line refuses those, and what the slices add is that
    they name the row, the mode and the channel."""
import pytest
import torch

from tests import spec_conv_cases as C


@pytest.mark.parametrize("name", [c.name for c in C.ALL_CASES], ids=[c.id for c in C.ALL_CASES])
def test_float32_oracle_stays_under_the_floor(name):
    case = C.CASE[name]
    inp, ref64, ref32 = C.references(name)
    q, nonzero = C.quantities(case, ref32, ref64, inp)
    assert not nonzero and all(v < C.FLOOR for v in q.values()), (q, nonzero)
    assert not C.failures(case, ref32, ref32, ref64, inp, who="ref32")        # (the TOL_COMP rows are 0 here by construction)


@pytest.mark.parametrize("name", ["overlap A", "axis 3d dead planes", "axis m3 B", "stream B2"])
def test_kept_set_and_zero_masks_are_the_operators(name):
    """ref64 against itself: every error 0, nothing off the kept set beyond float64 rounding, and the structurally zero
    gradients exactly zero - in both dtypes; the masks are not empty where the case was chosen for them"""
    case = C.CASE[name]
    inp, ref64, ref32 = C.references(name)
    q, nonzero = C.quantities(case, ref64, ref64, inp)
    assert not nonzero and q.pop("y:leak") < 1e-14 and q.pop("y:leak/bin") < 1e-14 and all(v == 0 for v in q.values()), q
    dead = sum(int((~C.dw_live_mask(case, c)).sum()) for c in range(C.ncorner(case)))
    assert dead == {"overlap A": 4 * 6, "axis 3d dead planes": 4 * 2 * 3 * 3}.get(name, 0)
    m = C.kept_mask(case)
    lead = 1
    for d in case.live[:-1]:
        lead *= 2 * d
    # the mirrors: rows m .. of bin 0 (and of the Nyquist bin where it is kept) that only the Hermitian part fills
    assert int(m.sum()) >= min(lead, int(torch.tensor(case.dims[:-1]).prod())) * case.live[-1]
    assert bool(m[(0,) * m.dim()])


# ---------------------------------------------------------------------------------------------------------------------
# planted faults, each in a float64 copy of the oracle's results: the fault is the whole error
# ---------------------------------------------------------------------------------------------------------------------
def _copy(ref64):
    return {k: ([t.clone() for t in v] if isinstance(v, list) else None if v is None else v.clone()) for k, v in ref64.items()}


def _blamed(name, plant, only):
    case = C.CASE[name]
    inp, ref64, ref32 = C.references(name)
    got = _copy(ref64)
    plant(case, inp, got)
    return C.blamed(C.failures(case, got, ref32, ref64, inp, who="planted", only=only))


def test_planted_mode_scale_is_refused_by_the_mode_slice_alone():
    """(a) one kept mode of y times 1 + 2e-5: 2e-5 / sqrt(714 kept modes) = 7.5e-7 of the whole tensor"""
    def plant(case, inp, got):
        sp = (2, 3)
        Y = torch.fft.rfftn(got["y"], dim=sp)
        Y[:, :, 5, 7] *= 1.0 + 2e-5
        got["y"] = torch.fft.irfftn(Y, s=case.dims, dim=sp)
    assert _blamed("stream B3", plant, ("y",)) == {"y/mode"}


def test_planted_row_copy_is_refused_by_the_row_slice():
    """(b) the last row of every 4-row block of sample 0 taken from the row above it, in y and in dx (what a clamped fetch of a
    partial block would do to every block): refused by the row slices - and by every other line (0.11 of the whole tensor)"""
    def plant(case, inp, got):
        for t in ("y", "dx"):
            v = got[t].reshape(case.B, -1, case.P, case.dims[-1])
            v[0, :, 3::4] = v[0, :, 2::4][:, :v[0, :, 3::4].shape[1]].clone()
            got[t] = v.reshape(got[t].shape)
    assert {"y/row", "dx/row"} <= _blamed("rows mfma rb4 partial", plant, ("y", "dx"))


def test_planted_single_row_passes_the_whole_tensor_line():
    """(b') ONE row of 2 x 2115 - the last row of the last, partial block of sample 1 - moved 1e-4 of the way to the row above
    it: 2.2e-6 of the whole tensor, under TOL_COMP, and 1.4e-4 of its own row"""
    def plant(case, inp, got):
        v = got["y"].reshape(case.B, -1, case.P, case.dims[-1])
        v[1, :, -1] += 1e-4 * (v[1, :, -2] - v[1, :, -1])
        got["y"] = v.reshape(got["y"].shape)
    blamed = _blamed("rows mfma rb4 partial", plant, ("y",))
    assert "y/row" in blamed and "y:TOL_COMP" not in blamed, blamed


def test_planted_stream_tail_is_refused_by_the_mode_slice():
    """(c) the last Ktot % 4 = 2 modes of the packed order (corner hi, row m - 1, bins 19 and 20: the partial last workgroup of a
    ceil(Ktot / 4) grid) summed over sample 0 only"""
    def plant(case, inp, got):
        assert case.Ktot % 4 == 2
        part = C.oracle_eval(case, inp, torch.float64, batch=slice(0, 1))["dw"][1]
        got["dw"][1][:, :, -1, -2:] = part[:, :, -1, -2:]
    blamed = _blamed("stream B3", plant, ("dw",))
    assert "dw1/mode" in blamed and not any(b.startswith("dw0") for b in blamed), blamed


def test_planted_input_channel_tail_is_refused_by_the_channel_slice():
    """(d) the last Cin % it = 40 % 16 = 8 input channels of dW zero"""
    def plant(case, inp, got):
        for w in got["dw"]:
            w[32:] = 0
    assert {"dw0/cin", "dw1/cin"} <= _blamed("gemm lds 40>64", plant, ("dw",))


def test_planted_leak_is_refused_by_the_bin_slice_alone():
    """(e) 1e-5 of one kept mode copied into a bin off the kept set (rows 17 .. 46 are not kept): the leak over ALL kept bins is
    1e-5 / sqrt(714) = 4e-7 and passes, the worst bin over the rms kept bin does not"""
    def plant(case, inp, got):
        sp = (2, 3)
        Y = torch.fft.rfftn(got["y"], dim=sp)
        Y[:, :, 20, 3] += 1e-5 * Y[:, :, 5, 3]
        got["y"] = torch.fft.irfftn(Y, s=case.dims, dim=sp)
    assert _blamed("stream B3", plant, ("y",)) == {"y:leak/bin"}


def test_comparison_rules():
    assert C.judge("c", "x", 1e-7, 1e-7) is None and C.judge("c", "x", 3e-6, 1e-7) is not None
    assert C.judge("c", "x", 0.0, 0.0) is None and C.judge("c", "x", float("nan"), 1e-7) is not None
    assert C.judge("c", "x", 4e-6, 0.0, fixed=C.TOL_COMP) is None and C.judge("c", "x", 6e-6, 0.0, fixed=C.TOL_COMP) is not None
    assert C.blamed([C.judge("c", "y/row", 1.0, 1e-7), C.judge("c", "y:TOL_COMP", 1.0, 0.0, fixed=C.TOL_COMP)]) == {"y/row", "y:TOL_COMP"}
