"""The Darcy loss without a GPU: the float64 restatement of tests/darcy_cases.py against the reference's own float32 results
(tests/golden/darcy_loss_small.npz), planted faults that the judged rows must refuse, the ABI's refusals, the datasets and the
Python surface."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import darcy_cases as K
from tests import judging

G = np.load(os.path.join(K.GOLDEN, "darcy_loss_small.npz"))
GOLDEN_LIMIT = 2e-6


@pytest.mark.parametrize("family,shape", K.GOLDEN_CASES)
def test_restatement_against_the_reference(family, shape):
    """field, loss_f and the gradient of the reference's float32 run within 2e-6 of the float64 restatement (its sliced
    FDM_Darcy and the pointwise form agree to rounding)"""
    inp = K.make_inputs(family, shape)
    ref64 = K.restated(inp["u"], inp["a"], None, None, torch.float64, g_f=1.0)
    pre = "{}_{}_{}/".format(family, *shape)
    rows = [("field", judging.rel_err(torch.from_numpy(G[pre + "field"]), ref64["field"])),
            ("loss_f", K.scalar_err(float(G[pre + "loss_f"]), ref64["loss_f"])),
            ("du", judging.rel_err(torch.from_numpy(G[pre + "du"]), ref64["grad"]))]
    lines = [f"{n:18s} reference32 {e:10.3e}   limit {GOLDEN_LIMIT:8.2e}" for n, e in rows]
    section = "host golden " + K.case_name(family, shape, y=False)
    for line in lines:
        print(section, line)
    K.LOG.replace(section, lines)
    bad = [line for (n, e), line in zip(rows, lines) if not e < GOLDEN_LIMIT]
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("family,shape", [("white", (3, 37)), ("darcy", (3, 37)), ("white", (2, 7))])
def test_float32_restatement_passes_its_own_rows(family, shape):
    inp, ref64, ref32 = K.references(family, shape, mol=True, y=True)
    assert not judging.rejected(K.loss_rows(ref32, ref64, ref32))


@pytest.mark.parametrize("fault", K.FAULTS)
def test_planted_fault_is_refused(fault):
    shape = (3, 37)
    inp, ref64, ref32 = K.references("white", shape, mol=True, y=True)
    bad = K.restated(*K.operands(inp, True, True), torch.float32, fault=fault)
    rows = K.loss_rows(bad, ref64, ref32)
    refused = judging.rejected(rows)
    K.LOG.replace(f"host fault {fault}", [f"{n:22s} faulty {e:10.3e}   ref32 {r:10.3e}   floor {f:7.1e}" for n, e, r, f in rows]
                  + ["refused: " + ", ".join(refused)])
    assert refused, f"{fault}: every row passed"


def test_corner_blocks_take_no_equation_gradient():
    inp, ref64, ref32 = K.references("white", (3, 37), mol=True, y=True)
    for ref in (ref64, ref32):
        assert not bool(K.corner_blocks(ref["grad_f"]).any())


def test_adjoint_is_autograds():
    """the explicit adjoint against autograd through the float64 restatement's forward, with the mollifier and the data term"""
    inp = K.make_inputs("white", (2, 7))
    out, a, y, mol = (t.double() for t in K.operands(inp, True, True))
    leaf = out.clone().requires_grad_(True)
    pred = leaf * mol
    res = K.residual(pred, a, 36.0 / 4.0) - 1.0
    loss_f = (res.reshape(2, -1).norm(dim=1) / 3).mean()
    loss_data = ((pred - y).reshape(2, -1).norm(dim=1) / y.reshape(2, -1).norm(dim=1)).mean()
    (K.DATA_WEIGHT * loss_data + loss_f).backward()
    ref = K.restated(out, a, y, mol, torch.float64)
    assert judging.rel_err(ref["grad"], leaf.grad) < 1e-14
    assert K.scalar_err(ref["loss_f"], loss_f.detach()) < 1e-15 and K.scalar_err(ref["loss_data"], loss_data.detach()) < 1e-15


# ---------------------------------------------------------------------------------------------------------------------
# the ABI without a GPU
# ---------------------------------------------------------------------------------------------------------------------
EINVAL, EUNSUPPORTED = -1, -2


@pytest.mark.parametrize("B,S,code,word", [(2, 4, EINVAL, "S=4"), (2, 0, EINVAL, "S=0"), (0, 61, EINVAL, "batch=0"),
                                           (-1, 61, EINVAL, "batch=-1"), (2, 4097, EUNSUPPORTED, "S=4097"),
                                           (2, 100000, EUNSUPPORTED, "S=100000")])
def test_abi_refuses_before_launching(B, S, code, word):
    from pde_policylearning_amd import _lib
    L = _lib.lib()
    buf = (C.c_float * 4)()
    p = C.cast(buf, C.c_void_p)
    for rc in (L.fno_darcy_loss_forward(B, S, p, None, p, p, p, p, p, 16, None),
               L.fno_darcy_loss_backward(B, S, p, None, p, p, None, None, p, p, 16, None)):
        assert rc == code
        assert word in L.fno_last_error().decode()


def test_abi_refuses_a_target_without_its_result():
    from pde_policylearning_amd import _lib
    L = _lib.lib()
    buf = (C.c_float * 4)()
    p = C.cast(buf, C.c_void_p)
    assert L.fno_darcy_loss_forward(2, 61, p, None, p, p, None, p, p, 16, None) == EINVAL
    msg = L.fno_last_error().decode()
    assert "y=0x" in msg and "loss_data=" in msg and "loss_data=0x" not in msg, msg
    assert L.fno_darcy_loss_forward(2, 61, p, None, p, None, p, p, p, 16, None) == EINVAL
    msg = L.fno_last_error().decode()
    assert "loss_data=0x" in msg and "y=" in msg and "y=0x" not in msg, msg


def test_limit_admits_the_full_grid():
    from pde_policylearning_amd import _lib
    from pde_policylearning_amd import functional as F
    assert F.DARCY_S_MAX >= 421 and _lib.lib().fno_darcy_loss_workspace_bytes(20, 421) > 0
    assert _lib.lib().fno_darcy_loss_workspace_bytes(1, F.DARCY_S_MAX) > 0
    assert _lib.lib().fno_darcy_loss_workspace_bytes(1, F.DARCY_S_MAX + 1) == 0


def test_workspace_bytes_grow():
    from pde_policylearning_amd import _lib
    L = _lib.lib()
    base = L.fno_darcy_loss_workspace_bytes(2, 61)
    assert base >= 2 * 57 * 57 * 4
    assert L.fno_darcy_loss_workspace_bytes(3, 61) > base
    assert L.fno_darcy_loss_workspace_bytes(2, 85) > base
    for b in (1, 2, 20):
        sizes = [L.fno_darcy_loss_workspace_bytes(b, s) for s in (5, 61, 141, 211, 421)]
        assert sizes[0] > 0 and sizes == sorted(set(sizes)), sizes
    assert all(n in _lib.EXPORTED_SYMBOLS for n in ("fno_darcy_loss_workspace_bytes", "fno_darcy_loss_forward", "fno_darcy_loss_backward"))


def test_tile_extent_is_the_headers():
    import re
    src = open(os.path.join(K.ROOT, "pde_policylearning_amd", "csrc", "k_darcy_loss.h")).read()
    assert int(re.search(r"constexpr int DARCY_T = (\d+);", src).group(1)) == K.T
    assert "atomic" not in src.replace("no atomics", "")


# ---------------------------------------------------------------------------------------------------------------------
# datasets and the Python surface
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mat(tmp_path_factory):
    import scipy.io
    path = str(tmp_path_factory.mktemp("darcy") / "darcy.mat")
    rng = np.random.default_rng(0)
    arrs = {"coeff": rng.uniform(3, 12, (6, 29, 29)), "sol": rng.uniform(-1, 1, (6, 29, 29))}
    scipy.io.savemat(path, arrs)
    return path, arrs


def test_darcy_flow_reads_a_mat_file(mat):
    from pde_policylearning_amd.libs.pino_utils.datasets import DarcyFlow
    from pde_policylearning_amd.libs.pino_utils.utils import torch2dgrid
    path, arrs = mat
    ds = DarcyFlow(path, nx=29, sub=4, offset=1, num=3)
    assert ds.S == 8 and len(ds) == 3 and ds.mesh.shape == (8, 8, 2) and ds.mesh.dtype == torch.float32
    x, u = ds[2]
    assert x.shape == (8, 8, 3) and u.shape == (8, 8) and x.dtype == torch.float32
    assert torch.equal(x[..., 0], torch.tensor(arrs["coeff"][3, ::4, ::4], dtype=torch.float))
    assert torch.equal(u, torch.tensor(arrs["sol"][3, ::4, ::4], dtype=torch.float))
    assert torch.equal(x[..., 1:], torch2dgrid(8, 8))
    assert float(ds.mesh[0, 0, 0]) == 0.0 and float(ds.mesh[-1, 0, 0]) == 1.0 and float(ds.mesh[0, -1, 1]) == 1.0
    assert torch.equal(ds.mesh[:, 3, 0], torch.linspace(0, 1, 8)) and torch.equal(ds.mesh[3, :, 1], torch.linspace(0, 1, 8))
    full = DarcyFlow(path, nx=29, sub=1, num=2)
    assert full.S == 29 and full[0][0].shape == (29, 29, 3)
    assert not x[..., 0].is_contiguous(), "a = x[..., 0] is a strided view: functional.darcy_loss copies it"


def test_darcy_combo_reads_a_mat_file_or_a_mapping(mat):
    from pde_policylearning_amd.libs.pino_utils.datasets import DarcyCombo
    path, arrs = mat
    for source in (path, arrs):
        ds = DarcyCombo(source, nx=29, sub=4, pde_sub=2, num=4, offset=2)
        assert (ds.S, ds.pde_S, len(ds)) == (8, 15, 4)
        assert ds.mesh.shape == (8, 8, 2) and ds.pde_mesh.shape == (15, 15, 2)
        data_ic, u, pde_ic = ds[1]
        assert data_ic.shape == (8, 8, 3) and u.shape == (8, 8) and pde_ic.shape == (15, 15, 3)
        assert torch.equal(pde_ic[..., 0], torch.tensor(arrs["coeff"][3, ::2, ::2], dtype=torch.float))
        assert torch.equal(data_ic[..., 0], pde_ic[::2, ::2, 0]) and torch.equal(pde_ic[..., 1:], ds.pde_mesh)
    assert DarcyCombo(arrs, nx=29, sub=1, pde_sub=1, num=2).pde_S == 29


def test_mollifier_is_the_loops():
    from pde_policylearning_amd.libs.pino_utils.train_2d import darcy_mollifier
    from pde_policylearning_amd.libs.pino_utils.utils import torch2dgrid
    m = darcy_mollifier(torch2dgrid(21, 21))
    assert m.dtype == torch.float32 and torch.equal(m, K.mollifier(21))
    assert bool((m[0] == 0).all()) and abs(float(m[10, 10]) - 0.001) < 1e-9


def test_cpu_inputs_are_refused(tmp_path, monkeypatch):
    from torch.utils.data import DataLoader
    from pde_policylearning_amd import functional as F
    from pde_policylearning_amd.libs.models.pino_models import FNO2d
    from pde_policylearning_amd.libs.pino_utils import losses
    from pde_policylearning_amd.libs.pino_utils.datasets import DarcyCombo, DarcyFlow
    from pde_policylearning_amd.libs.pino_utils.eval_2d import eval_burgers, eval_darcy
    from pde_policylearning_amd.libs.pino_utils.train_2d import train_2d_operator
    monkeypatch.chdir(tmp_path)
    u, a = torch.zeros(2, 7, 7), torch.ones(2, 7, 7)
    for call in (lambda: F.darcy_loss(u, a), lambda: F.darcy_loss(u, a, u, torch.ones(7, 7)), lambda: F.darcy_residual(u, a),
                 lambda: losses.darcy_loss(u, a), lambda: losses.FDM_Darcy(u, a)):
        with pytest.raises(RuntimeError, match="GPU"):
            call()
    assert not F.darcy_loss_supported(u)
    with pytest.raises(NotImplementedError, match="D=2"):
        losses.FDM_Darcy(u, a, D=2)
    model = FNO2d(modes1=[2, 2], modes2=[2, 2], fc_dim=8, layers=[4] * 3)
    opt = torch.optim.Adam(model.parameters())
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=10)
    arrs = {"coeff": np.ones((2, 13, 13)), "sol": np.ones((2, 13, 13))}
    for ds in (DarcyCombo(arrs, nx=13, sub=4, pde_sub=2, num=2), DarcyFlow(arrs, nx=13, sub=2, num=2)):
        with pytest.raises(RuntimeError, match="GPU"):
            train_2d_operator(model, DataLoader(ds, batch_size=2), opt, sched, K.TRAIN_CFG, rank="cpu", use_tqdm=False)
    with pytest.raises(RuntimeError, match="GPU"):
        eval_darcy(model, DataLoader(DarcyFlow(arrs, nx=13, sub=2, num=2), batch_size=2), None, "cpu", use_tqdm=False)
    with pytest.raises(RuntimeError, match="GPU"):
        eval_burgers(model, [(torch.zeros(2, 5, 32, 3), torch.zeros(2, 5, 32))], 0.01, None, "cpu", use_tqdm=False)
    assert not os.path.exists("checkpoints")
