"""Hostile dynamic range.  Every other parity input is a uniform [-1, 1) hash fill (oracle/detfill.py); the two-term fp16 GEMMs
(fno_dev.h "h2") keep full relative precision only for elements above 2^-16 of the PUBLISHED bound of their tensor, and at
|u| ~ 1 a missing or stale bound (scale 1) is nearly as good as the right one.  Here the magnitudes move: one channel 10^4 times
the others, heavy-tailed (log-normal) fields, an all-zero sample, a tensor whose maximum sits in a single element, one sample
whose target norm is 1e-6 (its LpLoss gradient is 1e6 x its batch mates': the outlier dy drives the gradient-bound chain of the
whole backward pass), a lifting 1e5 or 1e-3 times larger with block 0's weights scaled back (u_0 far from 1, block 1 unchanged).

The model cases run on every block-0 dispatch row of the fused model (ROWS: launch_block_x3 / launch_bbwd_c in fno_abi.hip), each
at a batch where B x pixels >= 2^17, so the two-term mode is on; every case asserts from the library's per-launch profile that the
pass ran the intended mode (block 0's backward with two fp16 terms on the rows whose kernels carry them, never where u_0 is
stored), and that the 64 bound slots
at the end of the forward's `saved` buffer hold what their consumers assume (_check_bound_slots: slot map from fno_abi.hip).

Reference: the oracle in float64 on float64 copies of the same float32 numbers; tolerance 1e-5 relative L2 on the output
(BASELINE.json north_star), gradients within the budget of tests/test_parity_gpu.py (1e-5, or BUDGET_SLACK x the float32
oracle's own distance from float64 where that is larger).  Outputs are held to plain 1e-5 wherever the float32 oracle itself is
under 5e-6; every case appends its achieved numbers (engine / float32 oracle against float64, per tensor) to the error table
that _record writes - the committed tables are profiles/r07_hostile_errors.txt (every row) and r06_hostile_errors.txt (round 6:
the strip row alone)."""
import os
import numpy as np
import pytest
import torch

from oracle import fno_oracle as O
from oracle.detfill import fill_named
from tests.judging import TOL_Y, dev  # noqa: F401
from tests.test_parity_gpu import _fno_params, _run_fused, _within_budget
from tests.util import rel_l2

pytestmark = pytest.mark.gpu
_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _record(test, case, name, e, e32):
    """one table row per (case, tensor): engine and float32-oracle distance from the float64 value"""
    try:
        os.makedirs(os.path.join(_ROOT, "gpurun_out"), exist_ok=True)
        with open(os.path.join(_ROOT, "gpurun_out", "hostile_errors.txt"), "a") as f:
            f.write(f"{test:12s} {case:22s} {name:40s} engine {e:.3e}   float32 oracle {e32:.3e}   ratio {e / max(e32, 1e-30):6.2f}\n")
    except OSError:
        pass


def _check_output(case, ey, ey32):
    # plain 1e-5 wherever the float32 evaluation of the reference is itself comfortably inside it; otherwise twice its distance
    assert np.isfinite(ey) and ey < (TOL_Y if ey32 < 5e-6 else max(TOL_Y, 2.0 * ey32)), (case, ey, ey32)


def _hostile(case, B, dims, C, L, half, cin=3):
    p = _fno_params(C, L, half, cin=cin)
    x = torch.from_numpy(fill_named("hx", (B, cin) + tuple(dims), 1.0))
    tgt = torch.from_numpy(fill_named("ht", (B, 1) + tuple(dims), 1.0))
    nw = 2 ** (len(dims) - 1)                 # spectral weight corners per block; block 0's are convs.weight.0 .. nw-1
    if case == "hidden_channel_x1e4":
        # ONE hidden channel 10^4 times the others after the lifting; block 0 reads it back with 10^-4 weights, so the sums
        # stay O(1) while the operand tile's maximum is 10^4 x its typical element
        c = 7
        p["lifting.fc.weight"][c] *= 1e4
        p["lifting.fc.bias"][c] *= 1e4
        p["fno_blocks.fno_skips.0.weight"][:, c] *= 1e-4
        for i in range(nw):
            p[f"fno_blocks.convs.weight.{i}.tensor"][c] *= 1e-4
    elif case in ("lift_x1e5", "lift_x1e-3"):
        # the WHOLE lifting f times larger, block 0's skip and spectral weights 1/f: block 0's pre-activation is unchanged, max |u_0|
        # is f x its usual O(1) - the two-term block-0 backward splits u_0 by the bound the forward published (slot 8): without it
        # (scale 1) the high fp16 term overflows at 1e5 and the low term underflows at 1e-3
        f, fi = (1e5, 1e-5) if case == "lift_x1e5" else (1e-3, 1e3)
        p["lifting.fc.weight"] *= f
        p["lifting.fc.bias"] *= f
        p["fno_blocks.fno_skips.0.weight"] *= fi
        for i in range(nw):
            p[f"fno_blocks.convs.weight.{i}.tensor"] *= fi
    elif case == "input_channel_x1e4":
        x[:, 1] *= 1e4
        p["lifting.fc.weight"][:, 1] *= 1e-4
    elif case == "lognormal":
        g = torch.Generator().manual_seed(11)
        x = torch.exp(2.5 * torch.randn(x.shape, generator=g)) * torch.sign(torch.randn(x.shape, generator=g))
        x = (x / x.abs().mean()).float()
    elif case == "zero_sample":
        x[1] = 0.0
    elif case == "single_spike":
        x *= 1e-3
        x[2, 0, 17, 93] = 1e3
    elif case == "tiny":
        x *= 1e-6
    elif case == "target_norm_1e-6":
        tgt[min(3, B - 1)] *= 1e-6      # dL/dy of that sample is 1e6 x the other samples' (LpLoss divides by the target's norm)
    else:
        raise ValueError(case)
    return p, x, tgt


# Block-0 dispatch rows of the fused model: (grid, width, n_modes, B, input channels, layers, lifting fused into block 0, block 0's
# backward two-term).  B x pixels >= 2^17 on every row (the two-term threshold of model_forward_impl).  What each row launches for
# block 0 (launch_block_x3 / launch_bbwd_c, fno_abi.hip; confirmed with a kernel trace of one pass per row):
#   strip          128^2, 64 ch, 12 modes    fwd k_blk_fwd_s<false, 2, true>                    bwd k_block_bwd_g2<true, false, 1, 2, true>
#   w64_rows64     64^2 (rows of 64)         fwd k_blk_fwd_t<64, true, false, false, 2, false, 1, 3>   bwd k_block_bwd_g2<true, false, 1, 2, true>
#   w64_rows32     32^2 (rows of 32)         fwd k_blk_fwd_t<64, true, false, false, 2, false, 1, 3>   bwd k_block_bwd_t<64, 128, false, true, false, 3>
#                                            (the g2 tile of 32-pixel rows exceeds LDS: every block backward is three-term here)
#   w64_many_bins  128^2, 24 modes, cin 4    fwd k_pw_fwd_x3<64, 128, 2, false, true> (12 kept last-dim bins > 8)
#                                            bwd k_block_bwd_t<64, 128, false, true, false, 3> (blocks above 0: k_block_bwd<64, 128>)
#   w32            128^2, 32 ch              fwd k_pw_fwd_x3<32, 128, 2, false, true>          bwd k_block_bwd_t<32, 128, false, true, false, 2>
#   fno3d_w32      32^3, 32 ch (BASELINE config-4 family)   fwd k_pw_fwd_x3<32, 128, 2, false, true>   bwd k_block_bwd_t<32, 128, false, true, false, 2>
#   unfused_lift   256^2: 256-pixel tiles, the lifting is its own launch (k_pw_fwd<3, 64, 256>) and u_0 is stored
#                                            fwd k_pw_fwd_x3<64, 256, 2>                        bwd k_block_bwd<64, 256> (fp32)
#                  (one layer: at 64 channels the plan refuses 256-pixel tiles of blocks that also carry the forward table)
#   loose          96^2: loose rows, the lifting is its own launch (k_pw_fwd<3, 64, 128>)
#                                            fwd k_pw_fwd_x3<64, 128, 2, true>                  bwd k_block_bwd_t<64, 128, true, false, false, 3>
ROWS = {
    "strip": ((128, 128), 64, (12, 12), 8, 3, 4, True, True),
    "w64_rows64": ((64, 64), 64, (12, 12), 32, 3, 3, True, True),
    "w64_rows32": ((32, 32), 64, (8, 8), 128, 3, 3, True, False),
    "w64_many_bins": ((128, 128), 64, (24, 24), 8, 4, 3, True, False),
    "w32": ((128, 128), 32, (12, 12), 8, 3, 3, True, True),
    "fno3d_w32": ((32, 32, 32), 32, (8, 8, 8), 4, 3, 3, True, True),
    "unfused_lift": ((256, 256), 64, (12, 12), 2, 3, 1, False, False),
    "loose": ((96, 96), 64, (12, 12), 16, 3, 3, False, False),
}
STRIP_CASES = ["hidden_channel_x1e4", "input_channel_x1e4", "lognormal", "zero_sample", "single_spike", "tiny",
               "target_norm_1e-6", "lift_x1e5", "lift_x1e-3"]
ROW_CASES = ["lift_x1e5", "lift_x1e-3", "target_norm_1e-6", "input_channel_x1e4"]
MODEL_CASES = [pytest.param("strip", c, id=c) for c in STRIP_CASES] + \
              [pytest.param(r, c, id=f"{r}-{c}") for r in ROWS if r != "strip" for c in ROW_CASES]


def _rel(a, b):
    return abs(a - b) / max(abs(b), 1e-300)


def _check_bound_slots(slots, ref, L, fused, npx128):
    """The 64 magnitude-bound slots at the end of `saved` after forward + backward, against the float64 tensors their consumers
    split (the host names them kBndX, bnd_u(l), bnd_g(l), kBndProj.. in fno_abi.hip; the literal numbers here are the independent
    statement of that map).  [7] max |x| (k_lift_rowdft, fused lifting);
    [8] the derived bound of |u_0| (block 0's forward, fused lifting); [8 + l] max |u_l| as stored, l = 1..L (before the GELU
    gate); [32 + l] max |dL/du_l|, l = 1..L (the gradient chain: the projection backward and the block backwards publish their
    gout, which is the gradient AFTER the GELU derivative of the stored u_l; [32 + L] is the two-term projection backward's, the
    blocks' are 0 where the launched kernel publishes none - the first-generation k_block_bwd - and the host then hands the next
    kernel no bound); [60] max |dy|, [61] max |W1|, [62] max |w2| (k_absmax3_pack_w1, two-term projection backward).  Every
    other slot stays 0.  Returns a list of failures."""
    bad = []
    used = set()

    def chk(i, lo, hi, what):
        used.add(i)
        s = float(slots[i])
        if ref_zero(what):
            if s != 0.0:
                bad.append(f"slot {i} ({what}) = {s:.6e}, its tensor is all zero")
        elif not (np.isfinite(s) and lo <= s <= hi):
            bad.append(f"slot {i} ({what}) = {s:.6e}, expected in [{lo:.6e}, {hi:.6e}]")

    def ref_zero(what):
        return what in ref and ref[what] == 0.0

    def near(i, what, tol):
        t = ref[what]
        chk(i, t * (1 - tol), t * (1 + tol), what)

    def band(i, what):
        t = ref[what]
        chk(i, 0.5 * t, 2.0 * t, what)

    if fused:
        near(7, "x", 1e-5)
        # the bound block 0's forward derived from slot 7 and the lifting parameters (k_blk_fwd_s's formula), on the host
        host = float(np.max(np.abs(ref["lw"]).sum(axis=1) * float(slots[7]) + np.abs(ref["lb"])))
        chk(8, max(ref["u0"] * (1 - 1e-6), host * (1 - 1e-6)), host * (1 + 1e-6), "u0")
    for l in range(1, L + 1):
        near(8 + l, f"u{l}", 1e-5)
    for l in range(1, L + 1):
        if (npx128 and l == L) or slots[32 + l] != 0.0:
            band(32 + l, f"g{l}")
    if npx128:
        band(60, "dy")
        band(61, "w1")
        band(62, "w2")
    for i in range(64):
        if i not in used and slots[i] != 0.0:
            bad.append(f"slot {i} = {float(slots[i]):.6e}, no producer in the slot map")
    return bad


@pytest.mark.parametrize("row,case", MODEL_CASES)
def test_fno_model_hostile_dynamic_range(dev, row, case):
    from pde_policylearning_amd import _lib
    dims, C, modes, B, cin, L, fused, bwd0_h2 = ROWS[row]
    npx128 = dims[-1] <= 128
    p, x, tgt = _hostile(case, B, dims, C, L, [m // 2 for m in modes], cin)
    torch.set_num_threads(min(torch.get_num_threads(), 16))
    p64 = {k: v.double().clone().requires_grad_(True) for k, v in p.items()}
    y64, u64 = O.fno_forward(p64, x.double(), modes, n_layers=L, return_intermediates=True, preact=True)
    for t in u64 + [y64]:
        t.retain_grad()
    O.lp_loss_rel_sum(y64, tgt.double()).backward()
    ref = {"x": float(x.abs().max()), "lw": p["lifting.fc.weight"].double().reshape(C, cin).numpy(),
           "lb": p["lifting.fc.bias"].double().numpy(), "dy": float(y64.grad.abs().max()),
           "w1": float(p["projection.fc1.weight"].abs().max()), "w2": float(p["projection.fc2.weight"].abs().max())}
    for l, t in enumerate(u64):
        ref[f"u{l}"] = float(t.detach().abs().max())
        if l > 0:
            ref[f"g{l}"] = float(t.grad.abs().max())
    del u64
    p32 = {k: v.clone().requires_grad_(True) for k, v in p.items()}
    y32 = O.fno_forward(p32, x, modes, n_layers=L)
    O.lp_loss_rel_sum(y32, tgt).backward()

    lib = _lib.lib()
    lib.fno_profile_reset()
    lib.fno_profile_enable(1)
    try:
        y, pg = _run_fused(p, x, modes, dev, n_layers=L)
        saved = y.grad_fn.saved_tensors[1]          # the forward's `saved` buffer (bytes); its last 64 floats are the bound slots
        O.lp_loss_rel_sum(y, tgt.to(dev)).backward()
        torch.cuda.synchronize()
        terms = {n: t for n, _, _, t in _lib.profile_summary(with_terms=True)}
    finally:
        lib.fno_profile_enable(0)
        lib.fno_profile_reset()
    slots = saved[-64 * 4:].view(torch.float32).cpu().numpy().astype(np.float64)
    del saved

    tag = case if row == "strip" else f"{row}:{case}"
    fails = []
    ey, ey32 = rel_l2(y.detach().cpu().numpy(), y64.detach().numpy()), rel_l2(y32.detach().numpy(), y64.detach().numpy())
    _record("fno_model", tag, "y", ey, ey32)
    try:
        _check_output(case, ey, ey32)
    except AssertionError as e:
        fails.append(f"output: {e}")
    errs = {k: (rel_l2(pg[k].grad.cpu().numpy(), p64[k].grad.numpy()), rel_l2(p32[k].grad.numpy(), p64[k].grad.numpy())) for k in p}
    for k, (e, e32) in errs.items():
        _record("fno_model", tag, k, e, e32)
    for k, (e, e32) in errs.items():
        try:
            assert np.isfinite(e), (k, "non-finite gradient")
            _within_budget(e, e32, (case, k))
        except AssertionError as ex:
            fails.append(f"gradient: {ex}")
    # the intended arithmetic ran: a row that fell below the two-term threshold would pass these comparisons for nothing
    if not any(t == 2 for t in terms.values()):
        fails.append(f"mode: no kernel ran with two fp16 terms: {terms}")
    if bwd0_h2 and terms.get("k_block_bwd0") != 2:
        fails.append(f"mode: block 0's backward ran with {terms.get('k_block_bwd0')} terms, expected 2")
    if not bwd0_h2 and terms.get("k_block_bwd0") in (None, 2):
        fails.append(f"mode: block 0's backward ran with {terms.get('k_block_bwd0')} terms, expected 3 or 1")
    if terms.get("k_proj_fwd") != 2 or (npx128 and terms.get("k_proj_bwd") != 2):
        fails.append(f"mode: projection forward / backward terms {terms.get('k_proj_fwd')} / {terms.get('k_proj_bwd')}")
    fails += [f"bounds: {m}" for m in _check_bound_slots(slots, ref, L, fused, npx128)]
    assert not fails, "\n".join([f"{row} {case}:"] + fails)


@pytest.mark.parametrize("case,C", [pytest.param(c, C, id=c if C == 64 else f"{c}-w32") for C in (64, 32)
                                    for c in ["channel_x1e4", "lognormal", "zero_sample", "single_spike", "dy_outlier_sample"]])
def test_projection_head_hostile_dynamic_range(dev, case, C):
    """The standalone projection head (fno_projection_forward / _backward) at widths 64 and 32.  It has one arithmetic mode,
    three bf16 terms (k_proj_fwd_x3 / k_proj_bwd_t<C, 256, false>); the two-term <32> and <64> projection kernels of the model
    path run under the model cases above (w32, fno3d_w32: k_proj_fwd_w<32> / k_proj_bwd_t<32, 256, false, 2>)."""
    from pde_policylearning_amd import _lib
    from pde_policylearning_amd import functional as F
    hid, shape = 256, (8, C, 128, 128)
    x = torch.from_numpy(fill_named("hpx", shape, 1.0))
    w1 = torch.from_numpy(fill_named("hpw1", (hid, C), 0.15))
    b1 = torch.from_numpy(fill_named("hpb1", (hid,), 0.1))
    w2 = torch.from_numpy(fill_named("hpw2", (1, hid), 0.1))
    b2 = torch.from_numpy(fill_named("hpb2", (1,), 0.1))
    dy = torch.from_numpy(fill_named("hpd", (shape[0], 1) + shape[2:], 1.0))
    if case == "channel_x1e4":
        x[:, 5] *= 1e4
        w1[:, 5] *= 1e-4
    elif case == "lognormal":
        g = torch.Generator().manual_seed(12)
        x = (torch.exp(2.5 * torch.randn(shape, generator=g)) * torch.sign(torch.randn(shape, generator=g))).float()
        x = x / x.abs().mean()
        w1 *= 0.05
    elif case == "zero_sample":
        x[3] = 0.0
        dy[5] = 0.0
    elif case == "dy_outlier_sample":
        dy[2] *= 1e6            # one sample's output gradient 1e6 x the others' (what a target of norm 1e-6 does to LpLoss)
    else:
        x *= 1e-3
        x[1, 9, 100, 3] = 1e3
    def ref(dtype):
        t = [v.to(dtype).clone().requires_grad_(True) for v in (x, w1, b1, w2, b2)]
        yr = (torch.nn.functional.gelu(t[0].movedim(1, -1) @ t[1].t() + t[2]) @ t[3].t() + t[4]).movedim(-1, 1)
        yr.backward(dy.to(dtype))
        return yr.detach().numpy(), [v.grad.numpy() for v in t]
    torch.set_num_threads(min(torch.get_num_threads(), 16))
    y64, g64 = ref(torch.float64)
    y32, g32 = ref(torch.float32)
    tag = case if C == 64 else f"w32:{case}"
    eng = [t.to(dev).requires_grad_(True) for t in (x, w1, b1, w2, b2)]
    lib = _lib.lib()
    lib.fno_profile_reset()
    lib.fno_profile_enable(1)
    try:
        ye = F.projection_head(*eng, act="gelu")
        ey, ey32 = rel_l2(ye.detach().cpu().numpy(), y64), rel_l2(y32, y64)
        _record("projection", tag, "y", ey, ey32)
        _check_output(case, ey, ey32)
        ye.backward(dy.to(dev))
        torch.cuda.synchronize()
        terms = {n: t for n, _, _, t in _lib.profile_summary(with_terms=True)}
    finally:
        lib.fno_profile_enable(0)
        lib.fno_profile_reset()
    assert terms.get("k_proj_fwd") == 3 and terms.get("k_proj_bwd") == 3, terms
    errs = [(name, rel_l2(a.grad.cpu().numpy(), r64), rel_l2(r32, r64)) for a, r64, r32, name in zip(eng, g64, g32, ("x", "w1", "b1", "w2", "b2"))]
    for name, e, e32 in errs:
        _record("projection", tag, name, e, e32)
    for name, e, e32 in errs:
        _within_budget(e, e32, (case, name))


@pytest.mark.parametrize("B", [9, 17])
def test_uneven_tile_shares_cover_every_tile(dev, B):
    """Two workgroups per CU split a CU's tiles unevenly (pair_share, fno_dev.h: the block forward's tiles, the projection
    forward's pixel columns popped from an LDS counter).  Batch sizes whose tile count is not a multiple of the grid
    (9 x 128 = 1152 and 17 x 128 = 2176 tiles on 512 workgroups: pairs own 4-5 or 8-9 tiles, split 2/2, 3/2, 4/4, 5/4) must
    still write every pixel exactly once: output and every gradient against float64."""
    S, C, L, modes = 128, 64, 4, (12, 12)
    p = _fno_params(C, L, [m // 2 for m in modes])
    x = torch.from_numpy(fill_named(f"ux{B}", (B, 3, S, S), 1.0))
    tgt = torch.from_numpy(fill_named(f"ut{B}", (B, 1, S, S), 1.0))
    torch.set_num_threads(min(torch.get_num_threads(), 16))
    p64 = {k: v.double().clone().requires_grad_(True) for k, v in p.items()}
    y64 = O.fno_forward(p64, x.double(), modes, n_layers=L)
    O.lp_loss_rel_sum(y64, tgt.double()).backward()
    p32 = {k: v.clone().requires_grad_(True) for k, v in p.items()}
    O.lp_loss_rel_sum(O.fno_forward(p32, x, modes, n_layers=L), tgt).backward()
    y, pg = _run_fused(p, x, modes, dev, n_layers=L)
    assert rel_l2(y.detach().cpu().numpy(), y64.detach().numpy()) < TOL_Y
    O.lp_loss_rel_sum(y, tgt.to(dev)).backward()
    torch.cuda.synchronize()
    for k in p:
        g64 = p64[k].grad.numpy()
        _within_budget(rel_l2(pg[k].grad.cpu().numpy(), g64), rel_l2(p32[k].grad.numpy(), g64), (B, k))
