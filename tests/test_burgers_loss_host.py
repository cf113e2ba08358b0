"""The Burgers loss without a GPU: the float64 restatement of tests/burgers_cases.py against the reference's own float32
results (tests/golden/burgers_loss_small.npz), planted faults that the judged rows must refuse, the ABI's refusals and the
Python surface."""
import ctypes as C
import os
import pickle

import numpy as np
import pytest
import torch

from tests import burgers_cases as K
from tests import judging

G = np.load(os.path.join(K.GOLDEN, "burgers_loss_small.npz"))
GM = np.load(os.path.join(K.GOLDEN, "pino_fno2d_small.npz"))


def _golden(family, shape):
    pre = "{}_{}_{}_{}/".format(family, *shape)
    return {"loss_u": torch.tensor(float(G[pre + "loss_u"])), "loss_f": torch.tensor(float(G[pre + "loss_f"])),
            "field": torch.from_numpy(G[pre + "field"]), "grad": torch.from_numpy(G[pre + "du"])}


@pytest.mark.parametrize("family,shape", K.GOLDEN_CASES)
def test_restatement_against_the_reference(family, shape):
    """white: losses, field and du of the reference within 2e-6 of the float64 restatement; smooth: the stored field within
    1.75 x 7e-6 and the losses within 2e-6 (D2 r amplifies rounding in the high bins of the smooth du: logged, with its
    projection onto the first 16 bins)."""
    inp, ref64, ref32 = K.references(family, shape, K.GOLDEN_VISC)
    got = _golden(family, shape)
    rows = [("field", judging.rel_err(got["field"], ref64["field"])), ("loss_f", K.scalar_err(got["loss_f"], ref64["loss_f"])),
            ("loss_u", K.scalar_err(got["loss_u"], ref64["loss_u"])), ("du", judging.rel_err(got["grad"], ref64["grad"])),
            ("du low 16 bins", judging.rel_err(K.low_bins(got["grad"]), K.low_bins(ref64["grad"])))]
    limits = {"field": 2e-6 if family == "white" else 1.75 * 7e-6, "loss_f": 2e-6, "loss_u": 2e-6}
    if family == "white":
        limits["du"] = 2e-6
    lines = [f"{n:18s} reference32 {e:10.3e}   limit {limits[n]:8.2e}" if n in limits else f"{n:18s} reference32 {e:10.3e}   logged"
             for n, e in rows]
    section = "host golden " + K.case_name(family, shape, K.GOLDEN_VISC)
    for line in lines:
        print(section, line)
    K.LOG.replace(section, lines)
    bad = [line for (n, e), line in zip(rows, lines) if n in limits and not e < limits[n]]
    assert not bad, "\n".join(bad)


def test_float32_restatement_passes_its_own_rows():
    inp, ref64, ref32 = K.references("white", (3, 11, 128), 0.01)
    assert not judging.rejected(K.loss_rows(ref32, ref64, ref32))


@pytest.mark.parametrize("fault", K.FAULTS)
def test_planted_fault_is_refused(fault):
    shape = (3, 11, 128)
    inp, ref64, ref32 = K.references("white", shape, 0.01)
    bad = K.restated(inp["u"], inp["u0"], 0.01, torch.float32, fault=fault)
    rows = K.loss_rows(bad, ref64, ref32)
    refused = judging.rejected(rows)
    K.LOG.replace(f"host fault {fault}", [f"{n:22s} faulty {e:10.3e}   ref32 {r:10.3e}   floor {f:7.1e}" for n, e, r, f in rows]
                  + ["refused: " + ", ".join(refused)])
    assert refused, f"{fault}: every row passed"


# ---------------------------------------------------------------------------------------------------------------------
# the ABI without a GPU
# ---------------------------------------------------------------------------------------------------------------------
EINVAL, EUNSUPPORTED = -1, -2


@pytest.mark.parametrize("B,nt,nx,code,word", [(2, 5, 48, EUNSUPPORTED, "nx=48"), (2, 5, 256, EUNSUPPORTED, "nx=256"),
                                               (2, 5, 31, EINVAL, "nx=31"), (2, 2, 32, EINVAL, "nt=2"), (0, 5, 32, EINVAL, "batch=0")])
def test_abi_refuses_before_launching(B, nt, nx, code, word):
    from pde_policylearning_amd import _lib
    L = _lib.lib()
    buf = (C.c_float * 4)()
    p = C.cast(buf, C.c_void_p)
    for rc in (L.fno_burgers_loss_forward(B, nt, nx, p, p, 0.01, p, p, p, 16, None),
               L.fno_burgers_loss_backward(B, nt, nx, p, p, 0.01, None, None, p, p, 16, None)):
        assert rc == code
        assert word in L.fno_last_error().decode()


def test_workspace_bytes_grow():
    from pde_policylearning_amd import _lib
    L = _lib.lib()
    base = L.fno_burgers_loss_workspace_bytes(2, 11, 64)
    assert base > 0
    assert L.fno_burgers_loss_workspace_bytes(3, 11, 64) > base
    assert L.fno_burgers_loss_workspace_bytes(2, 12, 64) > base
    assert L.fno_burgers_loss_workspace_bytes(2, 11, 128) > base
    sizes = [L.fno_burgers_loss_workspace_bytes(b, nt, nx) for b in (1, 2, 20) for nt in (3, 11, 101) for nx in (32, 64, 128)]
    assert all(s > 0 for s in sizes) and sizes[-1] == max(sizes)
    assert "fno_burgers_loss_forward" in _lib.EXPORTED_SYMBOLS and "fno_burgers_loss_backward" in _lib.EXPORTED_SYMBOLS


# ---------------------------------------------------------------------------------------------------------------------
# the Python surface
# ---------------------------------------------------------------------------------------------------------------------
def _model(**kw):
    from pde_policylearning_amd.libs.models.pino_models import FNO2d
    args = dict(modes1=list(K.MODES1), modes2=list(K.MODES2), fc_dim=128, layers=[32] * 4, in_dim=3, act="gelu")
    args.update(kw)
    return FNO2d(**args)


def test_fno2d_state_dict_is_the_references():
    sd = _model().state_dict()
    want = {k[len("shapes/"):]: tuple(int(s) for s in GM[k]) for k in GM.files if k.startswith("shapes/")}
    assert len(want) == 20
    assert {k: tuple(v.shape) for k, v in sd.items()} == want
    assert all(sd[k].is_complex() == ("sp_convs" in k) for k in sd)


def test_fno2d_layers_none_builds():
    m = _model(layers=None, width=32)
    assert m.layers == [32] * 4 and m.fc1.in_features == 32 and m.fc3.out_features == 1


def test_fno2d_pickles():
    m = _model(pad_ratio=[0., 0.125])
    m2 = pickle.loads(pickle.dumps(m))
    assert all(torch.equal(a, b) for a, b in zip(m.state_dict().values(), m2.state_dict().values()))
    assert m2.pad_ratio == [0., 0.125]


def test_fno2d_unknown_act():
    with pytest.raises(ValueError, match="swish is not supported"):
        _model(act="swish")


def test_cpu_inputs_are_refused():
    from pde_policylearning_amd import functional as F
    from pde_policylearning_amd.libs.pino_utils.losses import FDM_Burgers, PINO_loss
    with pytest.raises(RuntimeError, match="GPU"):
        _model()(torch.zeros(K.MODEL_X))
    u, u0 = torch.zeros(2, 5, 32), torch.zeros(2, 32)
    with pytest.raises(RuntimeError, match="GPU"):
        PINO_loss(u, u0, 0.01)
    with pytest.raises(RuntimeError, match="GPU"):
        FDM_Burgers(u, 0.01)
    assert not F.burgers_loss_supported(u)


def test_lploss_and_fdm_refusals():
    from pde_policylearning_amd.libs.pino_utils.losses import FDM_Burgers, LpLoss
    with pytest.raises(NotImplementedError, match="p=1"):
        LpLoss(p=1)
    with pytest.raises(NotImplementedError, match="reduction=False"):
        LpLoss(reduction=False)
    with pytest.raises(NotImplementedError, match="abs"):
        LpLoss().abs(torch.zeros(2, 4), torch.zeros(2, 4))
    with pytest.raises(NotImplementedError, match="D=2"):
        FDM_Burgers(torch.zeros(2, 5, 32), 0.01, D=2)


def test_save_checkpoint(tmp_path, monkeypatch):
    from pde_policylearning_amd.libs.pino_utils.utils import save_checkpoint
    monkeypatch.chdir(tmp_path)
    m = torch.nn.Linear(2, 2)
    save_checkpoint("run", "a.pt", m)
    save_checkpoint("run", "b.pt", m, torch.optim.Adam(m.parameters()))
    a, b = torch.load("checkpoints/run/a.pt"), torch.load("checkpoints/run/b.pt")
    assert a["optim"] == 0.0 and set(a["model"]) == {"weight", "bias"} and "param_groups" in b["optim"]
