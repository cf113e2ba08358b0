"""functional/_core.py's operand check and shape rules, driven on the CPU (no engine call is made here).

_operand is the one check between a tensor and its address; it reads only the anchor's device, so CPU tensors (and `meta`
tensors as "another device") exercise every refusal.  The tiling table and the GELU masks below are written out by hand from
the rules, not computed by the functions under test."""
import pytest
import torch

from pde_policylearning_amd import functional as F


def _refused(match_entry, match_name, **kw):
    with pytest.raises(RuntimeError) as ei:
        F._operand(match_entry, match_name, **kw)
    msg = str(ei.value)
    assert match_entry in msg and match_name in msg, msg
    return msg


def test_operand_accepts_and_returns_contiguous():
    x = torch.zeros(2, 4, 8)
    w = torch.arange(12, dtype=torch.float32).reshape(3, 4).t()               # (4, 3), not contiguous
    assert not w.is_contiguous()
    out = F._operand("entry", "w", w, x, numel=12, shape=(4, 3))
    assert out.is_contiguous() and torch.equal(out, w) and out.shape == (4, 3)
    good = torch.ones(4, 3)
    assert F._operand("entry", "w", good, x, numel=12) is good                   # nothing to copy
    assert F._operand("entry", "bias", None, x, optional=True) is None
    seed = torch.zeros(2, dtype=torch.int32)
    assert F._operand("entry", "seed", seed, x, dtype=torch.int32, numel=2) is seed
    m = torch.zeros(6, dtype=torch.float64)
    assert F._operand("entry", "metrics", m, x, dtype=torch.float64) is m
    assert F._operand("entry", "w", w, x, layout="keep") is w                    # corner weights keep their layout


def test_operand_refusals_name_entry_point_and_operand():
    x = torch.zeros(2, 4, 8)
    msg = _refused("fno_blocks", "skip weight 1", t=torch.zeros(4, 4, device="meta"), anchor=x)
    assert "meta" in msg and "cpu" in msg
    msg = _refused("fno_blocks", "bias", t=torch.zeros(4, dtype=torch.float64), anchor=x)
    assert "float32" in msg and "float64" in msg
    msg = _refused("fno_block_tail", "seed", t=torch.zeros(2, dtype=torch.int64), anchor=x, dtype=torch.int32)
    assert "int32" in msg and "int64" in msg
    msg = _refused("projection_head", "b1", t=torch.zeros(5), anchor=x, numel=4)
    assert "4 elements" in msg and "5" in msg
    msg = _refused("pointwise_conv_per_sample_bias", "bias", t=torch.zeros(4, 2), anchor=x, shape=(2, 4))
    assert "(2, 4)" in msg and "(4, 2)" in msg
    _refused("lifting_per_sample_bias", "bias", t=None, anchor=x)                # required, absent
    msg = _refused("adam_step", "grad", t=torch.zeros(4, 4).t()[:, :2], anchor=x, layout="dense")
    assert "contiguous" in msg


def test_corner_weight_front_door():
    x = torch.zeros(1, 2, 8, 8)
    good = [torch.zeros(2, 2, 3, 3, 2) for _ in range(2)]
    ws, planes = F._check_corner_weights("fno_blocks", good, x, 2, 2, (3, 3))
    assert not planes and all(a is b for a, b in zip(ws, good))
    with pytest.raises(RuntimeError, match="spectral weight 1") as ei:
        F._check_corner_weights("fno_blocks", [good[0], torch.zeros(2, 2, 2, 3, 2)], x, 2, 2, (3, 3))
    assert "fno_blocks" in str(ei.value) and "(2, 2, 3, 3, 2)" in str(ei.value)
    with pytest.raises(RuntimeError, match="spectral weight 0"):
        F._check_corner_weights("spectral_pointwise_layer", [w.double() for w in good], x, 2, 2, (3, 3))
    # the standalone plans state the stored last extent: it replaces modes[-1], plane-major or not
    pm = [F.to_plane_major(torch.zeros(2, 2, 3, 3, 5, dtype=torch.cfloat)) for _ in range(4)]
    rv = [torch.view_as_real(w) for w in pm]
    x3 = torch.zeros(1, 2, 8, 8, 8)
    ws, planes = F._check_corner_weights("spectral_conv", rv, x3, 2, 2, (3, 3, 4), last=5)
    assert planes and all(a is b for a, b in zip(ws, rv))
    with pytest.raises(RuntimeError, match="spectral weight"):
        F._check_corner_weights("spectral_conv", rv, x3, 2, 2, (3, 3, 4), last=6)


# (grid, tiled / loose / None in split-precision mode 1, the same in exact-fp32 mode 0).  By hand from the rule: tiled = last
# dim w a multiple of 32, <= 256, dividing the tile npx (256 pixels when w > 128, else 128), plane a multiple of npx; loose =
# not tiled, 32 <= w <= 320, plane a multiple of 128, split-precision mode only.
TILING = [
    ((128, 128), "tiled", "tiled"),
    ((64, 64), "tiled", "tiled"),
    ((256, 256), "tiled", "tiled"),
    ((96, 96), "loose", None),             # 128 % 96 != 0; 9216 = 72 * 128
    ((160, 160), "loose", None),           # 256 % 160 != 0; 25600 = 200 * 128
    ((128, 128, 73), "loose", None),       # 73 % 32 != 0; 128 * 128 * 73 is a multiple of 128
    ((128, 33), "loose", None),            # 33 % 32 != 0; 4224 = 33 * 128
    ((100, 33), None, None),               # 3300 % 128 != 0
    ((128, 31), None, None),               # below 32, not a multiple of 32
    ((128, 352), None, None),              # a multiple of 32 but above 256, and above 320
]


@pytest.mark.parametrize("dims,split,exact", TILING, ids=["x".join(map(str, t[0])) for t in TILING])
def test_row_tiling_table(dims, split, exact):
    assert F.row_tiling(dims, 1) == split
    assert F.row_tiling(dims, 0) == exact
    assert F.row_tiling(torch.Size(dims), 1) == split


def test_plane_size():
    assert F.plane_size((2, 3, 5, 7)) == 35 and F.plane_size(torch.Size((2, 3, 4, 5, 6))) == 120 and F.plane_size((2, 3, 9)) == 9


def test_default_gelu_mask():
    """the reference applies the activation after layer l while l < n_layers - l (fno_block.py:149)"""
    # L = 1: l = 0 < 1.  L = 2: 0 < 2, 1 < 1 no.  L = 3: 0 < 3, 1 < 2, 2 < 1 no.  L = 4: 0, 1 (1 < 3), 2 < 2 no.  L = 5: 0, 1, 2 (2 < 3)
    assert [F.default_gelu_mask(n) for n in (1, 2, 3, 4, 5)] == [0b1, 0b01, 0b011, 0b0011, 0b00111]


def test_cfg_record_names_its_fields():
    cfg = F._Cfg(2, (8, 8), "ortho", 0b01, tail=(True, 0.1, None))
    assert (cfg.n_layers, cfg.modes, cfg.norm, cfg.gelu_mask, cfg.direct, cfg.overlap, cfg.tail) == \
        (2, (8, 8), "ortho", 1, None, None, (True, 0.1, None))
