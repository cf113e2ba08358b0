"""Exact-fp32 GEMM mode (fno_set_gemm_mode(0): every channel GEMM on v_mfma_f32_32x32x2_f32) for the entry points the RNO
observer and the PINO heads are built from: the projection heads (fno_projection_*_act: GELU head with 1..PROJ_MAXCO outputs,
ReLU head) and the one-layer block with a ReLU tail and spectral-branch dropout (fno_model_*_tail).  Outputs within TOL_Y of
float64; gradients within 1e-5 of float64 or BUDGET_SLACK x the float32 reference's own distance from float64."""
import numpy as np
import pytest
import torch

from oracle import fno_oracle as O
from oracle import observers_oracle as OO
from oracle.detfill import fill_named
from tests.judging import BUDGET_SLACK, TOL_G, TOL_Y, dev  # noqa: F401
from tests.test_parity_gpu import _within_budget
from tests.util import rel_l2

pytestmark = pytest.mark.gpu

PROJ_MAXCO = 4


@pytest.fixture
def exact_mode():
    """The exact fp32 GEMM mode for the test, the previous mode restored after it."""
    from pde_policylearning_amd import _lib
    L = _lib.lib()
    prev = L.fno_get_gemm_mode()
    L.fno_set_gemm_mode(0)
    yield
    L.fno_set_gemm_mode(prev)


def _cpu(t):
    return t.detach().cpu().numpy()


def _profiled_terms(fn):
    """{kernel name: matrix-pipe terms} of the engine launches `fn` makes (fno_profile_get_terms: 1 = fp32 MFMA)."""
    from pde_policylearning_amd import _lib
    L = _lib.lib()
    L.fno_profile_reset()
    L.fno_profile_enable(1)
    try:
        out = fn()
        torch.cuda.synchronize()
        terms = {n: t for n, _, _, t in _lib.profile_summary(with_terms=True)}
    finally:
        L.fno_profile_enable(0)
        L.fno_profile_reset()
    return out, terms


def _assert_exact(terms):
    assert terms, "no engine launch recorded"
    split = {n: t for n, t in terms.items() if t not in (0, 1)}
    assert not split, f"split-precision kernels launched in the exact mode: {split}"


# ---------------------------------------------------------------------------
# 1. projection heads
# ---------------------------------------------------------------------------
def _head_ref(x, w1, b1, w2, b2, act, dy, dtype):
    t = [v.to(dtype).clone().requires_grad_(True) for v in (x, w1, b1, w2, b2)]
    actf = torch.nn.functional.gelu if act == "gelu" else torch.relu
    y = (actf(t[0].movedim(1, -1) @ t[1].t() + t[2]) @ t[3].t() + t[4]).movedim(-1, 1)
    y.backward(dy.to(dtype))
    return y.detach().numpy(), [v.grad.numpy() for v in t]


@pytest.mark.parametrize("C", [32, 64])
@pytest.mark.parametrize("hid,act,cout", [(128, "gelu", 1), (256, "gelu", 1), (128, "gelu", 2), (256, "gelu", 2),
                                          (128, "gelu", PROJ_MAXCO), (256, "gelu", PROJ_MAXCO), (256, "relu", 1)])
def test_projection_head_exact_fp32_vs_float64(dev, exact_mode, C, hid, act, cout):
    from pde_policylearning_amd import functional as F
    shape = (2, C, 16, 24)
    x = torch.from_numpy(fill_named("xph.x", shape, 1.0))
    w1 = torch.from_numpy(fill_named("xph.w1", (hid, C), 0.15))
    b1 = torch.from_numpy(fill_named("xph.b1", (hid,), 0.1))
    w2 = torch.from_numpy(fill_named("xph.w2", (cout, hid), 0.1))
    b2 = torch.from_numpy(fill_named("xph.b2", (cout,), 0.1))
    dy = torch.from_numpy(fill_named("xph.dy", (shape[0], cout) + shape[2:], 1.0))
    assert F.projection_supported(x.to(dev), hid, cout, act)
    y64, g64 = _head_ref(x, w1, b1, w2, b2, act, dy, torch.float64)
    _, g32 = _head_ref(x, w1, b1, w2, b2, act, dy, torch.float32)
    eng = [t.to(dev).requires_grad_(True) for t in (x, w1, b1, w2, b2)]
    y, tf = _profiled_terms(lambda: F.projection_head(*eng, act=act))
    _assert_exact(tf)
    assert rel_l2(_cpu(y), y64) < TOL_Y
    _, tb = _profiled_terms(lambda: y.backward(dy.to(dev)))
    _assert_exact(tb)
    for name, a, r64, r32 in zip(("dx", "dW1", "db1", "dW2", "db2"), eng, g64, g32):
        _within_budget(rel_l2(_cpu(a.grad), r64), rel_l2(r32, r64), name)


# ---------------------------------------------------------------------------
# 2. block tail: relu(specconv(drop(x)) + W x + b)
# ---------------------------------------------------------------------------
def _tail_ref(x, w, b, s0, s1, m, scale, mask, dy, dtype):
    """float64 / float32 oracle of the tail; `mask` (engine's ReLU decisions) imposed where given."""
    t = [v.to(dtype).clone().requires_grad_(True) for v in (x, w, b, s0, s1)]
    xs = t[0] if scale is None else t[0] * scale.to(dtype)
    spec = O.spectral_conv_B(xs, t[3], t[4], m, m)
    pre = spec + torch.einsum("oi,bixy->boxy", t[1], t[0]) + t[2][None, :, None, None]
    y = pre if mask is None else pre * mask.to(dtype)
    y.backward(dy.to(dtype))
    return y.detach().numpy(), pre.detach(), [v.grad.numpy() for v in t]


@pytest.mark.parametrize("C,S,m", [(32, 32, 6), (64, 32, 6), (32, 64, 8), (64, 64, 8), (32, 128, 12), (64, 128, 12)])
@pytest.mark.parametrize("relu_out", [True, False])
@pytest.mark.parametrize("drop_p", [0.0, 0.3])
def test_block_tail_exact_fp32_vs_float64(dev, exact_mode, C, S, m, relu_out, drop_p):
    from pde_policylearning_amd import functional as F
    B = 2
    x = torch.from_numpy(fill_named("xbt.x", (B, C, S, S), 1.0))
    w = torch.from_numpy(fill_named("xbt.w", (C, C), 1.0 / C ** 0.5))
    b = torch.from_numpy(fill_named("xbt.b", (C,), 0.1))
    s0 = torch.from_numpy(fill_named("xbt.s0", (C, C, m, m, 2), 1.0 / C))
    s1 = torch.from_numpy(fill_named("xbt.s1", (C, C, m, m, 2), 1.0 / C))
    dy = torch.from_numpy(fill_named("xbt.dy", (B, C, S, S), 1.0))
    assert F.block_tail_supported(x.to(dev), (m, m), "ortho")
    seed = F.draw_dropout_seed(dev) if drop_p > 0 else None
    eng = [t.to(dev).requires_grad_(True) for t in (x, w, b, s0, s1)]
    y, tf = _profiled_terms(lambda: F.fno_block_tail(eng[0], eng[1], [eng[3], eng[4]], eng[2].view(1, -1), (m, m), "ortho",
                                                     relu_out=relu_out, drop_p=drop_p, seed=seed))
    _assert_exact(tf)
    assert ("k_rowdft_tile_drop" in tf) == (drop_p > 0), tf
    # the oracles take the mask from the same seed words (a backward that regenerated another mask fails the gradients) and the
    # ReLU decisions from the engine's output (a float32 decision within rounding of zero is not an arithmetic error)
    scale = F.dropout_scale(x.numel(), drop_p, seed, dev).view(x.shape).cpu() if drop_p > 0 else None
    mask = (_cpu(y) > 0) if relu_out else None
    mask_t = torch.from_numpy(mask) if relu_out else None
    y64, pre64, g64 = _tail_ref(x, w, b, s0, s1, m, scale, mask_t, dy, torch.float64)
    _, _, g32 = _tail_ref(x, w, b, s0, s1, m, scale, mask_t, dy, torch.float32)
    if relu_out:
        flips = int(((pre64 > 0).numpy() != mask).sum())
        assert flips <= 1e-5 * mask.size, flips
        assert 0.2 < mask.mean() < 0.8
    assert rel_l2(_cpu(y), y64) < TOL_Y
    _, tb = _profiled_terms(lambda: y.backward(dy.to(dev)))
    _assert_exact(tb)
    for name, a, r64, r32 in zip(("dx", "dW", "db", "dspec0", "dspec1"), eng, g64, g32):
        got = _cpu(a.grad).reshape(r64.shape)
        _within_budget(rel_l2(got, r64), rel_l2(r32, r64), name)


# ---------------------------------------------------------------------------
# 3. / 4. whole models: the exact mode makes no more torch layer calls than the default mode
# ---------------------------------------------------------------------------
_COUNTED = ("linear", "conv1d", "conv2d", "conv3d", "relu", "dropout")      # (not gelu: the PINO heads test `act is TF.gelu`)


class _TorchCalls(object):
    """Counts calls of the torch.nn.functional layer ops (hipBLAS / MIOpen / elementwise kernels) while active."""

    def __enter__(self):
        self.n = dict.fromkeys(_COUNTED, 0)
        self.orig = {k: getattr(torch.nn.functional, k) for k in _COUNTED}
        for k, fn in self.orig.items():
            def wrapped(*a, _k=k, _fn=fn, **kw):
                self.n[_k] += 1
                return _fn(*a, **kw)
            setattr(torch.nn.functional, k, wrapped)
        return self

    def __exit__(self, *exc):
        for k, fn in self.orig.items():
            setattr(torch.nn.functional, k, fn)


class _EngineCalls(object):
    """Counts calls of the engine's tail / head entry points while active."""
    NAMES = ("fno_block_tail", "projection_head")

    def __enter__(self):
        from pde_policylearning_amd import functional as F
        self.F = F
        self.n = dict.fromkeys(self.NAMES, 0)
        self.orig = {k: getattr(F, k) for k in self.NAMES}
        for k, fn in self.orig.items():
            def wrapped(*a, _k=k, _fn=fn, **kw):
                self.n[_k] += 1
                return _fn(*a, **kw)
            setattr(F, k, wrapped)
        return self

    def __exit__(self, *exc):
        for k, fn in self.orig.items():
            setattr(self.F, k, fn)


def _counted_step(model, run, mode):
    from pde_policylearning_amd import _lib
    L = _lib.lib()
    prev = L.fno_get_gemm_mode()
    L.fno_set_gemm_mode(mode)
    try:
        with _TorchCalls() as tc, _EngineCalls() as ec:
            model.zero_grad(set_to_none=True)
            run()
            torch.cuda.synchronize()
    finally:
        L.fno_set_gemm_mode(prev)
    return tc.n, ec.n


def _head_decisions(head, a):
    """The decisions of the fused ReLU head (nn.Sequential(fc1, ReLU, fc2)) on its channels-first input `a`, as the kernel takes
    them in the exact-fp32 mode: (B, X, Y, hidden) bool on the CPU.  One hidden unit per call: second layer e_k, no bias."""
    from pde_policylearning_amd import _lib
    from pde_policylearning_amd import functional as F
    fc1 = head[0]
    hid = fc1.out_features
    L = _lib.lib()
    prev = L.fno_get_gemm_mode()
    L.fno_set_gemm_mode(0)
    try:
        out = torch.empty(a.shape[0], a.shape[2], a.shape[3], hid, dtype=torch.bool, device=a.device)
        b2 = torch.zeros(1, device=a.device)
        with torch.no_grad():
            for k in range(hid):
                w2 = torch.zeros(1, hid, device=a.device)
                w2[0, k] = 1.0
                out[..., k] = F.projection_head(a, fc1.weight.detach(), fc1.bias.detach(), w2, b2, act="relu")[:, 0] > 0
    finally:
        L.fno_set_gemm_mode(prev)
    return out.cpu()


def _compare(model, y, y64, g64, g32, gcond, slack):
    """As the full-size cfg-3 check: output within TOL_Y; every gradient within 1e-5 or slack x the larger of the float32
    oracle's and the conditioning floor (a one-number parameter is held to the worst floor of the model)."""
    assert rel_l2(_cpu(y).reshape(y64.shape), y64) < TOL_Y
    floor = {k: max(rel_l2(g32[k], g64[k]), rel_l2(gcond[k], g64[k])) for k in g64}
    top = max(floor.values())
    floor = {k: (top if g64[k].size == 1 else f) for k, f in floor.items()}
    for name, prm in model.named_parameters():
        got = prm.grad
        got = _cpu(torch.view_as_real(got) if got.is_complex() else got)
        e = rel_l2(got, g64[name])
        assert np.isfinite(got).all() and e < max(TOL_G, slack * floor[name]), (name, e, floor[name])


def test_rno2d_exact_mode_train_step_engine_only_vs_float64(dev):
    """RNO2d observer (BASELINE config 3's model: modes 12, width 64, one layer) at 128 x 128, batch 2, training mode with the
    regressor's dropout: in the exact mode the regressor's two Fourier layers (fused tails) and its ReLU head run on the engine,
    so the step makes no more torch layer calls than the default mode; and the exact-mode step matches float64 (the oracle takes
    the engine's dropout fields, from the same seed words, and its ReLU decisions).

    ALL of its ReLU decisions, the fused head's 2 x 128 x 128 x 256 included: that kernel never materialises its hidden tensor,
    so they are read out of it, one hidden unit per call, with a one-hot second layer (y = relu(hidden_k)).  Until round 10 the
    head was left to each evaluation's own decisions, and the comparison measured ties instead of arithmetic: torch's float32
    on the CPU decides 2 of the 8.4 M head inputs otherwise than float64, which alone puts 2e-5 .. 2e-4 on every gradient
    upstream of the head (and nothing on regressor.2), the exact-fp32 engine used to take the same two and so sat on the
    float32 oracle's figures to four digits, and a SELU that is 1e-5 more accurate (expm1) moved it to other ties and out of the
    budget.  With the head conditioned too, all three evaluations differentiate one function; how many
    of the engine's decisions differ from float64's own is bounded as in tests/test_fullsize_gpu.py."""
    from pde_policylearning_amd import functional as F
    from pde_policylearning_amd.libs.models.rno_models import RNO2dObserver
    torch.manual_seed(0)
    model = RNO2dObserver(12, 12, 64, 0, layer_num=1).train()
    params = {k: v.detach().clone() for k, v in model.state_dict().items()}
    x = torch.from_numpy(fill_named("xrno.x", (2, 1, 128, 128, 1), 1.0))
    tgt = torch.from_numpy(fill_named("xrno.t", (2, 128, 128, 1), 1.0))
    model = model.to(dev)
    xd, td = x.to(dev), tgt.to(dev)
    out = {}

    def step():
        y = model(xd)
        O.lp_loss_rel_sum(y, td.reshape(y.shape)).backward()
        out["y"] = y

    n1, e1 = _counted_step(model, step, 1)
    assert e1 == {"fno_block_tail": 2, "projection_head": 1}, e1
    # the exact-mode step, with its dropout seeds and ReLU decisions recorded for the oracle
    seeds, masks, head_in = [], {}, {}
    orig_seed = F.draw_dropout_seed
    F.draw_dropout_seed = lambda d: seeds.append(orig_seed(d)) or seeds[-1]
    for j, layer in enumerate(model.regressor.spectral_conv):
        def wrapped(a, _f=layer.forward_channels_first, _j=j):
            o = _f(a)
            masks[f"regressor.spectral_conv.{_j}"] = (o.detach() > 0).permute(0, 2, 3, 1).cpu()
            head_in[_j] = o.detach().clone()
            return o
        layer.forward_channels_first = wrapped
    try:
        (n0, e0), terms = _profiled_terms(lambda: _counted_step(model, step, 0))
    finally:
        F.draw_dropout_seed = orig_seed
        for layer in model.regressor.spectral_conv:
            del layer.forward_channels_first
    assert e0 == e1, e0
    assert all(n0[k] <= n1[k] for k in _COUNTED), (n0, n1)
    assert sum(n0.values()) == 0, n0
    _assert_exact(terms)
    assert len(seeds) == 2 and len(masks) == 2
    masks["regressor.head"] = _head_decisions(model.regressor.regressor, head_in[1])

    scales = [F.dropout_scale(2 * 64 * 128 * 128, 0.3, s, dev).view(2, 64, 128, 128).permute(0, 2, 3, 1).cpu() for s in seeds]
    orig_layer = OO.spectral_conv_with_fc

    def layer_with_dropout(p, t, m, tag="relu"):
        """rno.py:92-106 in training mode: the spectral branch sees drop(x), with the engine's scale field."""
        j = int(tag.rsplit(".", 1)[1])
        res = t @ p["linear.weight"].t() + p["linear.bias"]
        ys = O.spectral_conv_B((t * scales[j].to(t.dtype)).permute(0, 3, 1, 2), p["spec_conv.fourier_weight.0"],
                               p["spec_conv.fourier_weight.1"], m, m)
        return OO._relu(tag, ys.permute(0, 2, 3, 1) + res)

    def oracle(prm, xin, dtype):
        pc = {k: (v.to(dtype) if v.is_floating_point() else v).clone().requires_grad_(True) for k, v in prm.items()}
        OO.RELU_HOOK = hooks[dtype] = OO.ReluMasks(impose=masks)
        OO.spectral_conv_with_fc = layer_with_dropout
        try:
            y = OO.rno2d_forward(pc, xin.to(dtype), 12, 12, 64, 0, 1)
            O.lp_loss_rel_sum(y, tgt.to(dtype).reshape(y.shape)).backward()
        finally:
            OO.RELU_HOOK = None
            OO.spectral_conv_with_fc = orig_layer
        return y.detach().numpy(), {k: v.grad.numpy() for k, v in pc.items()}

    hooks = {}
    y64, g64 = oracle(params, x, torch.float64)
    # the oracle adopts the ENGINE's decisions, so the decisions themselves are checked (as tests/test_fullsize_gpu.py does)
    flips = {t: int((torch.cat(seen) != masks[t]).sum()) for t, seen in hooks[torch.float64].seen.items()}
    print("ReLU decisions of the engine that differ from the float64 oracle's own:", flips, "of", {t: m.numel() for t, m in masks.items()})
    assert set(flips) == set(masks) and sum(flips.values()) <= 1e-6 * sum(m.numel() for m in masks.values()), flips
    _, g32 = oracle(params, x, torch.float32)
    gen = torch.Generator().manual_seed(1)
    move = lambda v: v.double() * (1 + (torch.rand(v.shape, generator=gen, dtype=torch.float64) * 2 - 1) * 2.0 ** -24)
    _, gcond = oracle({k: move(v) for k, v in params.items()}, move(x), torch.float64)
    _compare(model, out["y"], y64, g64, g32, gcond, slack=BUDGET_SLACK)


def test_pino_plane_head_exact_mode_engine_only(dev):
    """PINObserverFullField's PlanePredHead (fc1 -> GELU -> fc2 onto out_dim * plane_num = 4 channels) at a whole-row shape:
    in the exact mode the multi-output head runs on the engine (no more torch layer calls than the default mode), and the
    two modes agree."""
    from pde_policylearning_amd.libs.models.pino_models import PINObserverFullField
    torch.manual_seed(4)
    model = PINObserverFullField(4, [4] * 4, [4] * 4, [4] * 4, width=64, fc_dim=128, in_dim=4, out_dim=1).to(dev)
    x = torch.randn(2, 16, 16, 32, 4, device=dev)
    re = torch.tensor([[180.0], [395.0]], device=dev)
    res = {}

    def step(tag):
        def run():
            y = model(x, re)
            y.square().sum().backward()
            res[tag] = [y.detach().clone()] + [p.grad.clone() for p in model.parameters()]
        return run

    n1, e1 = _counted_step(model, step(1), 1)
    assert e1["projection_head"] == 1, e1
    (n0, e0), terms = _profiled_terms(lambda: _counted_step(model, step(0), 0))
    assert e0 == e1, e0
    assert all(n0[k] <= n1[k] for k in _COUNTED), (n0, n1)
    _assert_exact({n: t for n, t in terms.items() if n in ("k_proj_fwd", "k_proj_bwd")})
    # (wiring check between the two fp32 evaluations; the kernels' numerics are held to float64 above)
    assert rel_l2(_cpu(res[0][0]), _cpu(res[1][0])) < 1e-5
    for (name, _), u, v in zip(model.named_parameters(), res[0][1:], res[1][1:]):
        u = torch.view_as_real(u) if u.is_complex() else u
        v = torch.view_as_real(v) if v.is_complex() else v
        assert rel_l2(_cpu(u), _cpu(v)) < (2e-2 if "sp_convs" in name else 5e-4), name
