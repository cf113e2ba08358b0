"""The one-dimensional spectral convolution (csrc/k_spec1d.h) and the FNO1d models on the GPU against float64 on the CPU.
Cases, references and the criterion: tests/fno1d_cases.py.  Before any number is compared every case asserts from the launch
log that the launches are the 1-D kernels and only those; every achieved error goes to profiles/r19_fno1d_errors.txt before
anything is asserted."""
import math

import pytest
import torch

from oracle import fno_oracle as O
from tests import fno1d_cases as K
from tests.judging import dev, judge_budget  # noqa: F401

pytestmark = pytest.mark.gpu

# profile labels of the 2-D / 3-D spectral path (k_channel_sums and k_pack_w1_x3 are not among them: the projection head
# launches those too)
OLD_SPECTRAL = ("k_rowdft", "k_rowidft", "k_axis", "k_mode_", "k_unpack_dw", "k_spec_mid")


def s1_route(cin, cout, backward=True):
    fwd = [f"k_s1_ana<{cin}>", "k_s1_mix_fwd", f"k_s1_syn<{cout}>"]
    return fwd + ([f"k_s1_ana<{cout}>", "k_s1_mix_bwd", f"k_s1_syn<{cin}>"] if backward else [])


def assert_route(records, want, only=True):
    """the 1-D launches are `want`, in order; only: nothing else was launched; otherwise: nothing of the 2-D / 3-D spectral path"""
    got = [r["variant"] for r in records if r["variant"].startswith("k_s1_")]
    assert got == want, [r["variant"] or r["name"] for r in records]
    if only:
        assert len(records) == len(want), [r["variant"] or r["name"] for r in records]
    assert not [r["name"] for r in records if r["name"].startswith(OLD_SPECTRAL) or r["name"] == "k_pack_w"], [r["name"] for r in records]
    for r in records:
        if r["variant"].startswith("k_s1_"):
            assert r["lds"] <= 64 * 1024 and r["block"] == (256, 1, 1), r


def conv_eval(case, inp, dev, grads=True):  # noqa: F811
    """forward (+ backward) of one case through functional.spectral_conv -> ({"y", "dx", "dw", "dbias"} on the CPU, records)"""
    from pde_policylearning_amd import _lib
    from pde_policylearning_amd import functional as F
    x = inp["x"].to(dev).requires_grad_(grads)
    w = inp["w"].to(dev).requires_grad_(grads)
    b = inp["bias"].to(dev).requires_grad_(grads) if inp["bias"] is not None else None
    with _lib.launch_log() as log:
        y = F.spectral_conv(x, [w], b, (case.M,), case.norm, weight_last_extent=case.wle)
        if grads:
            y.backward(inp["dy"].to(dev))
        torch.cuda.synchronize()
    out = {"y": y.detach().cpu()}
    if grads:
        out.update(dx=x.grad.cpu(), dw=w.grad.cpu()[..., :case.M], dbias=b.grad.cpu() if b is not None else None)
    return out, log.records


@pytest.mark.parametrize("name", [c.name for c in K.CASES])
def test_conv_vs_float64(dev, name):  # noqa: F811
    case, inp = K.CASE[name], K.inputs(name)
    got, records = conv_eval(case, inp, dev)
    assert_route(records, s1_route(case.cin, case.cout))
    slabs = math.ceil(case.N / 256)
    assert [r["grid"][:2] for r in records] == ([(slabs, case.B), (case.M, math.ceil(case.B / 16)), (slabs, case.B)]
                                                + [(slabs, case.B), (case.M, 1), (slabs, case.B)])
    judge_budget(K.LOG, name, K.rows(got, K.references(name)))


def test_strided_weight_leaves_the_dead_bins_alone(dev):  # noqa: F811
    """weight_last_extent 24, 12 kept: the gradient is written at the weight's stride and bins 12..23 of the caller's gradient
    storage keep what the caller left there (direct_grads writes into .grad in place)"""
    from pde_policylearning_amd import functional as F
    case, inp = K.CASE["A_strided_w"], K.inputs("A_strided_w")
    x = inp["x"].to(dev)
    w = inp["w"].to(dev).requires_grad_(True)
    w.grad = torch.full_like(w, complex(7.0, -3.0))
    y = F.spectral_conv(x, [w], None, (case.M,), case.norm, weight_last_extent=case.wle, direct_grads=True)
    y.backward(inp["dy"].to(dev))
    g = w.grad.cpu()
    assert bool((g[..., case.M:] == complex(7.0, -3.0)).all())
    ref = K.references("A_strided_w")
    judge_budget(K.LOG, "A_strided_w direct", K.rows({"dw": g[..., :case.M]}, ref))


@pytest.mark.parametrize("gelu", [False, True])
def test_layer_vs_float64(dev, gelu):  # noqa: F811
    """spectral_pointwise_layer: GELU while the slab is staged, and du through fno_pointwise_backward"""
    from pde_policylearning_amd import _lib
    from pde_policylearning_amd import functional as F
    case, inp = K.LAYER, K.inputs(K.LAYER.name)
    t = {k: inp[k].to(dev).requires_grad_(True) for k in ("x", "w", "pw", "bias")}
    assert F.spectral_layer_supported(t["x"], 1, (case.M,), case.norm, case.M, gelu)
    with _lib.launch_log() as log:
        y = F.spectral_pointwise_layer(t["x"], [t["w"]], (case.M,), case.norm, t["pw"], t["bias"], input_gelu=gelu)
        y.backward(inp["dy"].to(dev))
        torch.cuda.synchronize()
    assert_route(log.records, s1_route(case.cin, case.cout), only=False)
    got = {"y": y.detach().cpu(), "du": t["x"].grad.cpu(), "dw": t["w"].grad.cpu(), "dpw": t["pw"].grad.cpu(),
           "dbias": t["bias"].grad.cpu()}
    judge_budget(K.LOG, f"layer_gelu input_gelu={int(gelu)}", K.rows(got, K.layer_references(gelu)))


def test_off_band_cosine(dev):  # noqa: F811
    """a pure cosine at the first dropped bin: |y - bias| / |x| <= 1e-5 (a DFT by GEMM is orthogonal only to rounding)"""
    case, inp = K.CASE["A_one_tile"], dict(K.inputs("A_one_tile"))
    n = torch.arange(case.N, dtype=torch.float64)
    amp = torch.linspace(0.5, 2.0, case.B * case.cin, dtype=torch.float64).reshape(case.B, case.cin, 1)
    inp["x"] = (amp * torch.cos(2 * math.pi * case.M * n / case.N)).float()
    got, records = conv_eval(case, inp, dev, grads=False)
    assert_route(records, s1_route(case.cin, case.cout, backward=False))
    leak = float((got["y"] - inp["bias"].reshape(1, -1, 1)).double().norm() / inp["x"].double().norm())
    K.LOG.replace("off_band_cosine", [f"|y - bias| / |x| = {leak:.3e}   bound 1.0e-05"])
    assert leak <= 1e-5, leak


def test_bitwise_repeatable_and_batch_independent(dev):  # noqa: F811
    case, inp = K.CASE["C_three_tiles"], K.inputs("C_three_tiles")
    a, _ = conv_eval(case, inp, dev)
    b, _ = conv_eval(case, inp, dev)
    for k in ("y", "dx", "dw"):
        assert torch.equal(torch.view_as_real(a[k]) if a[k].is_complex() else a[k],
                           torch.view_as_real(b[k]) if b[k].is_complex() else b[k]), k
    one = {k: (v[1:2] if k in ("x", "dy") else v) for k, v in inp.items()}
    s, _ = conv_eval(case, one, dev)
    assert torch.equal(s["y"][0], a["y"][1]) and torch.equal(s["dx"][0], a["dx"][1])


def _model_eval(model, names, p, x, dy, dev):  # noqa: F811
    from pde_policylearning_amd import _lib
    inp = {n: p[n].to(dev).requires_grad_(True) for n in names}
    with _lib.launch_log() as log:
        y = torch.func.functional_call(model, inp, (x.to(dev),))
        grads = torch.autograd.grad(y, [inp[n] for n in names], dy.to(dev))
        torch.cuda.synchronize()
    return {"y": y.detach().cpu(), **{"grad " + n: g.cpu() for n, g in zip(names, grads)}}, log.records


@pytest.mark.parametrize("variant", ["four_layers", "one_layer", "incremental"])
def test_neuralop_fno1d_vs_float64(dev, variant):  # noqa: F811
    from pde_policylearning_amd.neuralop.models import FNO1d
    kw = {"four_layers": {}, "one_layer": {"n_layers": 1}, "incremental": {"incremental_n_modes": (8,)}}[variant]
    model = FNO1d(16, 32, in_channels=2, out_channels=1, **kw).to(dev)
    L, n_modes = model.n_layers, (8,) if variant == "incremental" else (16,)
    half = n_modes[0] // 2
    p = K.neuralop_params(model, "nop." + variant)
    x, dy = K._t(f"nop.{variant}.x", (2, 2, 256), 1.0), K._t(f"nop.{variant}.dy", (2, 1, 256), 1.0)
    names = list(p)
    got, records = _model_eval(model, names, p, x, dy, dev)
    want = []
    for l in range(L):
        want += s1_route(32, 32, backward=False)
    for l in range(L):
        want += s1_route(32, 32)[3:]
    assert_route(records, want, only=False)
    assert [r["name"] for r in records if r["name"].startswith(("k_lift", "k_proj"))], "lifting and projection run on the engine"
    # the oracle takes the live bins of the weights; the bins beyond them (incremental_n_modes) get no gradient
    wkeys = [n for n in names if "convs.weight" in n]
    for n in wkeys:
        assert not bool(got["grad " + n][:, :, half:].any()), n
        got["grad " + n] = got["grad " + n][:, :, :half]
    p_live = {n: (v[:, :, :half].contiguous() if n in wkeys else v) for n, v in p.items()}
    ref = K.model_reference(lambda q, xx: O.fno_forward(q, xx, n_modes, n_layers=L, fft_norm="forward"), p_live, x, dy)
    judge_budget(K.LOG, f"neuralop FNO1d {variant}", K.rows(got, ref))


@pytest.mark.parametrize("act", ["gelu", "relu"])
def test_pino_fno1d_vs_float64(dev, act):  # noqa: F811
    from pde_policylearning_amd.libs.models.pino_models import FNO1d
    modes = [12] * 3
    model = FNO1d(modes=modes, width=32, act=act).to(dev)
    p = K.pino_params(model, "pino." + act)
    x, dy = K._t(f"pino.{act}.x", (2, 128, 2), 1.0), K._t(f"pino.{act}.dy", (2, 128, 1), 1.0)
    names = list(p)
    got, records = _model_eval(model, names, p, x, dy, dev)
    want = []
    for l in range(3):
        want += s1_route(32, 32, backward=False)
    for l in range(3):
        want += s1_route(32, 32)[3:]
    assert_route(records, want, only=False)
    engine_glue = [r["name"] for r in records if r["name"].startswith(("k_lift", "k_proj", "k_pw"))]
    assert bool(engine_glue) == (act == "gelu"), engine_glue
    ref = K.model_reference(lambda q, xx: K.pino_fno1d_forward(q, xx, modes, act), p, x, dy)
    judge_budget(K.LOG, f"pino FNO1d act={act}", K.rows(got, ref))


@pytest.mark.parametrize("which", ["neuralop", "pino_gelu", "pino_relu"])
def test_second_step_through_a_direct_write_bucket_is_a_fresh_gradient(dev, which):  # noqa: F811
    """trainer.FlatGradBucket(direct_module=model) marks the model's engine-written gradients and never clears them: after two
    steps on different data every p.grad must be the SECOND step's gradient, not the sum of both.  Held to 1e-6 relative L2
    against a fresh evaluation of step 2 without a bucket: the engine's part is bitwise repeatable, the torch glue (Conv1d
    backward) is free to reorder its sums, and a gradient that kept step 1 is off by the size of step 1's gradient."""
    from pde_policylearning_amd.trainer import FlatGradBucket
    from tests.judging import rel_err
    if which == "neuralop":
        from pde_policylearning_amd.neuralop.models import FNO1d
        make = lambda: FNO1d(16, 32, in_channels=2, out_channels=1)      # noqa: E731
        shape_x, shape_y, params = (2, 2, 256), (2, 1, 256), K.neuralop_params
    else:
        from pde_policylearning_amd.libs.models.pino_models import FNO1d
        make = lambda: FNO1d(modes=[12] * 3, width=32, act=which[5:])      # noqa: E731
        shape_x, shape_y, params = (2, 128, 2), (2, 128, 1), K.pino_params
    models = [make(), make()]
    p = params(models[0], "bucket." + which)
    for m in models:
        m.load_state_dict(p)
        m.to(dev)
    data = [(K._t(f"bucket.{which}.x{i}", shape_x, 1.0).to(dev), K._t(f"bucket.{which}.dy{i}", shape_y, 1.0).to(dev)) for i in (1, 2)]
    bucket = FlatGradBucket(models[0].parameters(), direct_module=models[0])
    for x, dy in data:
        bucket.zero()
        models[0](x).backward(dy)
    names = [n for n, _ in models[1].named_parameters()]
    fresh = torch.autograd.grad(models[1](data[1][0]), [q for _, q in models[1].named_parameters()], data[1][1])
    got = dict(models[0].named_parameters())
    re = lambda t: torch.view_as_real(t.resolve_conj()) if t.is_complex() else t      # noqa: E731
    errs = {n: rel_err(re(got[n].grad).cpu(), re(f).cpu()) for n, f in zip(names, fresh)}
    K.LOG.replace(f"bucket second step {which}", [f"{n:40s} step-2 gradient vs fresh {e:.3e}   bound 1.0e-06" for n, e in errs.items()])
    assert max(errs.values()) <= 1e-6, errs


def test_uncovered_grid_is_refused_before_any_launch(dev):  # noqa: F811
    from pde_policylearning_amd import _lib
    from pde_policylearning_amd.neuralop.models import FNO1d
    model = FNO1d(16, 32).to(dev)
    with _lib.launch_log() as log:
        with pytest.raises(RuntimeError, match=r"\(2, 3, 100\)"):
            model(torch.zeros(2, 3, 100, device=dev))
    assert log.records == []
