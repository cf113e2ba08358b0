"""FNO blocks with the channel MLP (use_mlp=True), the part that needs no GPU: the float32 restatement against the reference's
stored results, the module surface, every refusal, and the C ABI's argument checks (tests/channel_mlp_cases.py)."""
import ctypes
import io
import pickle

import pytest
import torch

from tests import channel_mlp_cases as K
from tests.judging import TOL_COMP, rel_err

GOLDEN_CASES = [c for c, v in K.MODEL_CASES.items() if v[4] is not None]


@pytest.fixture(scope="module")
def lib():
    from pde_policylearning_amd import build, _lib
    build.build()
    return _lib.lib()


@pytest.mark.parametrize("cname", GOLDEN_CASES)
def test_restatement_matches_the_reference_float32(cname):
    """the reading of fno_block.py / mlp.py / skip_connections.py in tests/channel_mlp_cases.py, evaluated in float32, against
    what the reference itself computed: output and every parameter gradient"""
    p, x, g = K.model_params(cname)
    got = K.model_reference(cname, p, x, torch.float32)
    rows = [("y", rel_err(got["y"], torch.from_numpy(g["y"])))]
    rows += [(n, rel_err(got[n], torch.from_numpy(g["grads/" + n]).reshape(got[n].shape))) for n in p]
    for n, e in rows:
        print(f"{cname} {n:44s} {e:.3e}")
    assert set(k[len("grads/"):] for k in g.files if k.startswith("grads/")) == set(p)
    bad = [(n, e) for n, e in rows if not e < TOL_COMP]
    assert not bad, bad


@pytest.mark.parametrize("cname", GOLDEN_CASES)
def test_state_dict_matches_the_reference(cname):
    _, _, g = K.model_params(cname)
    sd = K.build_model(cname).state_dict()
    want = {k[len("shapes/"):]: tuple(int(s) for s in g[k]) for k in g.files if k.startswith("shapes/")}
    assert {k: tuple(v.shape) for k, v in sd.items()} == want
    L = K.MODEL_CASES[cname][2]["n_layers"]
    for l in range(L):
        assert f"fno_blocks.mlp.{l}.fcs.0.weight" in sd and f"fno_blocks.mlp.{l}.fcs.1.bias" in sd
        assert torch.equal(sd[f"fno_blocks.mlp_skips.{l}.weight"], torch.ones_like(sd[f"fno_blocks.mlp_skips.{l}.weight"]))


def test_constructor_surface_and_pickle():
    from pde_policylearning_amd.neuralop.models import FNO, FNO2d, FNO3d
    from pde_policylearning_amd.neuralop.models.fno_block import SoftGating
    m = FNO2d(12, 12, 64, use_mlp=True)
    blk = m.fno_blocks
    assert len(blk.mlp) == 4 and len(blk.mlp_skips) == 4 and blk.mlp[0].hidden_channels == 32
    assert blk.mlp[0].fcs[0].weight.shape == (32, 64, 1, 1) and blk.mlp[0].fcs[1].weight.shape == (64, 32, 1, 1)
    assert blk.mlp_skips[0].weight.shape == (1, 64, 1, 1)
    assert [blk.gelu_after(l) for l in range(4)] == [True, True, False, False]      # the path without an MLP keeps its rule
    assert FNO2d(12, 12, 64).fno_blocks.mlp is None
    # FNO2d / FNO3d do not forward mlp_skip (it lands in **kwargs, as `skip` does): always soft-gating through them
    assert isinstance(FNO2d(4, 4, 64, use_mlp=True, mlp_skip='identity', skip='linear').fno_blocks.mlp_skips[0], SoftGating)
    m3 = FNO3d(4, 4, 4, 32, use_mlp=True, mlp_expansion=1.0)
    assert m3.fno_blocks.mlp[1].fcs[0].weight.shape == (32, 32, 1, 1, 1) and m3.fno_blocks.mlp_skips[1].weight.shape == (1, 32, 1, 1, 1)
    ident = FNO((4, 4), 64, use_mlp=True, mlp_expansion=1.0, mlp_skip='identity')
    assert isinstance(ident.fno_blocks.mlp_skips[0], torch.nn.Identity)
    assert not any("mlp_skips" in k for k in ident.state_dict())
    assert not m.fused_supported(torch.zeros(1, 3, 32, 32))
    buf = io.BytesIO()
    pickle.dump(m, buf)
    m2 = pickle.loads(buf.getvalue())
    sd, sd2 = m.state_dict(), m2.state_dict()
    assert type(m2) is type(m) and list(sd) == list(sd2) and all(torch.equal(sd[k], sd2[k]) for k in sd)


@pytest.mark.parametrize("what, build", [
    ("width 32 at expansion 0.5 (H = 16)", lambda M: M.FNO((8, 8), 32, use_mlp=True)),
    ("width 48", lambda M: M.FNO2d(8, 8, 48, use_mlp=True)),
    ("width 64 at expansion 2", lambda M: M.FNO2d(8, 8, 64, use_mlp=True, mlp_expansion=2.0)),
    ("mlp_dropout", lambda M: M.FNO2d(8, 8, 64, use_mlp=True, mlp_dropout=0.1)),
    ("mlp_skip", lambda M: M.FNO((8, 8), 64, use_mlp=True, mlp_skip='linear')),
    ("norm", lambda M: M.FNO2d(8, 8, 64, use_mlp=True, norm="group_norm")),
    ("norm", lambda M: M.FNO2d(8, 8, 64, norm="group_norm")),
    ("preactivation", lambda M: M.FNO2d(8, 8, 64, use_mlp=True, preactivation=True)),
])
def test_what_the_kernel_does_not_cover_is_refused(what, build):
    from pde_policylearning_amd.neuralop import models as M
    with pytest.raises(NotImplementedError) as e:
        build(M)
    if what in ("mlp_dropout", "mlp_skip", "norm", "preactivation"):
        assert what in str(e.value)
    else:
        assert "mlp" in str(e.value)


def test_cpu_tensors_are_refused_naming_the_gpu():
    from pde_policylearning_amd import functional as F
    t = K.op_inputs(K.OP_CASES[0])
    with pytest.raises(RuntimeError, match="GPU"):
        F.channel_mlp(t["u"], t["x"], t["w1"], t["b1"], t["w2"], t["b2"], t["gate"], True)
    assert not F.channel_mlp_supported(t["u"], 32)
    m = K.build_model("fno2d_mlp_small")
    with pytest.raises(RuntimeError, match="GPU"):
        m(torch.zeros(2, 3, 16, 32))
    with pytest.raises(RuntimeError, match="GPU"):
        m.fno_blocks(torch.zeros(2, 64, 16, 32), 0)


def test_get_model_builds_the_mlp_configuration():
    """neuralop/tests/test_config.yaml's shape of a model section (use_mlp: 1, mlp: {expansion, dropout}, skip), at a width the
    kernel covers; `mlp` and `skip` land in **kwargs as in the reference (model_dispatcher.py -> tfno.py:449)"""
    from pde_policylearning_amd.neuralop.models import FNO2d, get_model
    cfg = {"arch": "fno2d",
           "fno2d": dict(data_channels=3, n_modes_height=8, n_modes_width=8, hidden_channels=64, projection_channels=32, n_layers=2,
                         domain_padding=0, domain_padding_mode='symmetric', fft_norm='forward', norm=None, skip='soft-gating',
                         implementation='factorized', use_mlp=1, mlp=dict(expansion=0.5, dropout=0), factorization=None, rank=1.0,
                         fixed_rank_modes=None, joint_factorization=False),
           "patching": {"levels": 0}}
    m = get_model(cfg)
    assert type(m) is FNO2d and len(m.fno_blocks.mlp) == 2 and m.fno_blocks.mlp[0].hidden_channels == 32
    assert m.projection.fc1.weight.shape == (32, 64, 1, 1)


def test_abi_refuses_bad_arguments_without_a_launch(lib):
    """bad widths, a plane that is no multiple of 128, null required pointers and a short workspace: an error code each, and
    nothing is launched (this machine has no GPU: a launch would be a HIP error, code FNO_EHIP, or a crash on the fake addresses)"""
    from pde_policylearning_amd import _lib
    vp = ctypes.c_void_p
    P = vp(0x1000)      # never dereferenced: every call below must return before a launch
    fwd = lambda B, C, H, pw, ptrs: lib.fno_channel_mlp_forward(B, C, H, pw, *ptrs[:7], 1, ptrs[7], None)  # noqa: E731
    bwd = lambda B, C, H, pw, ptrs, ws, n: lib.fno_channel_mlp_backward(B, C, H, pw, *ptrs[:7], 1, *ptrs[7:15], ws, n, None)  # noqa: E731
    ok8, ok15 = [P] * 8, [P] * 15
    with _lib.launch_log() as log:
        for C, H in ((64, 16), (32, 16), (32, 64), (48, 32), (64, 128), (128, 64)):
            assert lib.fno_channel_mlp_workspace_bytes(C, H, 2, 256) == 0
            assert fwd(2, C, H, 256, ok8) < 0 and bwd(2, C, H, 256, ok15, P, 1 << 30) < 0
        for C, H in K.WIDTHS:
            need = lib.fno_channel_mlp_workspace_bytes(C, H, 2, 256)
            assert need > 0
            assert lib.fno_channel_mlp_workspace_bytes(C, H, 2, 200) == 0 and lib.fno_channel_mlp_workspace_bytes(C, H, 0, 256) == 0
            assert fwd(2, C, H, 200, ok8) < 0 and bwd(2, C, H, 200, ok15, P, need) < 0
            assert b"128" in lib.fno_last_error()
            for i in (0, 1, 2, 3, 4, 5, 7):                       # u x w1 b1 w2 b2 [gate] y
                assert fwd(2, C, H, 256, [None if j == i else P for j in range(8)]) < 0, i
                assert b"null" in lib.fno_last_error()
            for i in (0, 1, 2, 3, 4, 5, 7, 8, 10, 11, 12, 13):    # u x w1 b1 w2 b2 [gate] dy du [dx] dw1 db1 dw2 db2 [dgate]
                assert bwd(2, C, H, 256, [None if j == i else P for j in range(15)], P, need) < 0, i
                assert b"null" in lib.fno_last_error()
            assert bwd(2, C, H, 256, ok15, None, need) < 0
            assert bwd(2, C, H, 256, [None if j == 14 else P for j in range(15)], P, need) < 0        # gate without dgate
            assert bwd(2, C, H, 256, [None if j == 6 else P for j in range(15)], P, need) < 0         # dgate without gate
            assert bwd(2, C, H, 256, ok15, P, need - 256) < 0
            assert b"workspace" in lib.fno_last_error()
            # the workspace follows the launch: fewer tiles than CUs need fewer partial slabs
            assert lib.fno_channel_mlp_workspace_bytes(C, H, 1, 128) < need
    assert log.records == []
