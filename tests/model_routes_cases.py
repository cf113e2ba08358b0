"""The route every model class takes at the smallest shape that reaches each rung (a helper module, not a conftest): the case
table shared by tools/model_routes.py, which prints launches and output bits per case, and tests/test_model_routes_gpu.py, which
holds every case to EXPECTED.  tools/model_routes.py loads this file by path, so that it can run the cases on another checkout's
package: nothing here imports the package before run_case does.

A case: cls "module:Class" below pde_policylearning_amd, constructor args / kw, the input shape `x` (as the class takes it),
`re` (the model takes a per-sample Reynolds number), `grad_x` (the input asks for its gradient), `attrs` (set on every
submodule before the run), `bucket` (the run goes through trainer.FlatGradBucket(direct_module=model)).

EXPECTED: case -> (the rungs layer_stack.run took, in call order; the engine's kernel names of one forward + backward, in launch
order, repeats folded as `N*[ ... ]`, see expand; "refused": the forward raises RuntimeError).  The kernel names were recorded at the commit before layer_stack existed (profiles/r23_model_routes_parent.txt); a pull
request that moves a model to another rung changes this table in its diff.  Grids are left out: they follow the CU count."""
import hashlib
import importlib

_PINO = dict(fc_dim=128, in_dim=1, out_dim=1, pad_ratio=[0.0, 0.0])
_FF = "libs.models.pino_models.pinobserver:PINObserverFullField"
_P2D = "libs.models.pino_models.pinobserver:PINObserver2d"
_M = "neuralop.models:"


def _ff(width, modes, grid, act="gelu", layers=None, **kw):
    layers = layers or [width] * 5
    return dict(cls=_FF, args=[2], kw=dict(_PINO, modes1=[modes[0]] * 4, modes2=[modes[1]] * 4, modes3=[modes[2]] * 4, layers=layers,
                                            act=act, **kw), x=(2,) + grid + (1,), re=True)


def _p2d(grad_x, pad):
    return dict(cls=_P2D, args=[], kw=dict(_PINO, modes1=[4] * 4, modes2=[4] * 4, modes3=[3] * 4, layers=[32] * 5, in_dim=4, act="gelu",
                                           pad_ratio=pad), x=(2, 16, 16, 16, 4), re=True, grad_x=grad_x)


CASES = {
    # PlanePredHead inside PINObserverFullField
    "planes chain": _ff(32, (4, 4, 3), (16, 16, 9)),
    "planes fused loose rows": _ff(64, (4, 8, 8), (8, 16, 73)),
    "planes relu addend": _ff(32, (4, 4, 3), (16, 16, 9), act="relu"),
    "planes mixed widths": _ff(32, (4, 4, 3), (16, 16, 9), layers=[32, 32, 64, 64, 64]),
    "planes width 16": _ff(16, (4, 4, 3), (16, 16, 9)),
    "planes no_engine_tail": dict(_ff(32, (4, 4, 3), (16, 16, 9)), attrs={"no_engine_tail": True}),
    "policy grad_x": dict(cls="libs.models.pino_models.pinobserver:PolicyModel2D", args=[],
                          kw=dict(_PINO, modes1=[4] * 4, modes2=[4] * 4, modes3=[3] * 4, layers=[32] * 5, act="gelu", zero_init=False),
                          x=(2, 16, 16, 9, 1), re=True, grad_x=True),
    # PINObserver2d: the per-sample-bias whole-forward route (no input gradient, B <= 16) and the other
    "observer2d per-sample": _p2d(False, [0.0, 0.0]),
    "observer2d per-sample padded": _p2d(False, 0.0625),
    "observer2d grad_x": _p2d(True, [0.0, 0.0]),
    "observer2d grad_x padded": _p2d(True, 0.0625),
    # neuralop FNO
    "fno2d whole model": dict(cls=_M + "FNO2d", args=[8, 8, 32], kw={}, x=(2, 3, 32, 32), grad_x=True),
    "fno2d width 16": dict(cls=_M + "FNO2d", args=[8, 8, 16], kw={}, x=(2, 3, 32, 32), grad_x=True),
    "fno2d padded fused": dict(cls=_M + "FNO2d", args=[8, 8, 32], kw=dict(domain_padding=1.0 / 3.0), x=(2, 3, 48, 48), grad_x=True),
    "fno2d padded per layer": dict(cls=_M + "FNO2d", args=[8, 8, 32], kw=dict(domain_padding=0.25), x=(2, 3, 32, 32), grad_x=True),
    "fno2d mlp": dict(cls=_M + "FNO2d", args=[8, 8, 64], kw=dict(use_mlp=True), x=(2, 3, 32, 32), grad_x=True),
    "fno2d mlp padded": dict(cls=_M + "FNO2d", args=[8, 8, 64], kw=dict(use_mlp=True, domain_padding=1.0 / 3.0), x=(2, 3, 48, 48)),
    "fno2d mlp composition": dict(cls=_M + "FNO2d", args=[8, 8, 64], kw=dict(use_mlp=True), x=(2, 3, 16, 24)),
    "fno2d incremental direct": dict(cls=_M + "FNO2d", args=[8, 8, 32], kw=dict(incremental_n_modes=(4, 4)), x=(2, 3, 32, 32),
                                     bucket=True),
    "fno2d direct": dict(cls=_M + "FNO2d", args=[8, 8, 32], kw={}, x=(2, 3, 32, 32), bucket=True),
    "fno3d": dict(cls=_M + "FNO3d", args=[8, 8, 8, 32], kw={}, x=(1, 3, 16, 16, 16), grad_x=True),
    "fno3d padded": dict(cls=_M + "FNO3d", args=[8, 8, 8, 32], kw=dict(domain_padding=1.0), x=(1, 3, 16, 16, 16)),
    "fno1d": dict(cls=_M + "FNO1d", args=[16, 32], kw={}, x=(2, 3, 128), grad_x=True),
    "fno1d padded": dict(cls=_M + "FNO1d", args=[16, 32], kw=dict(domain_padding=0.5), x=(2, 3, 256), grad_x=True),
    "fno1d one layer": dict(cls=_M + "FNO1d", args=[16, 32], kw=dict(n_layers=1), x=(2, 3, 128)),
    # the PINO models
    "pino fno1d": dict(cls="libs.models.pino_models:FNO1d", args=[[8, 8, 8]], kw=dict(act="gelu"), x=(2, 128, 2)),
    "pino fno1d relu": dict(cls="libs.models.pino_models:FNO1d", args=[[8, 8, 8]], kw=dict(act="relu"), x=(2, 128, 2)),
    "pino fno1d fc_dim 64": dict(cls="libs.models.pino_models:FNO1d", args=[[8, 8, 8]], kw=dict(act="gelu", fc_dim=64), x=(2, 128, 2)),
    "pino fno2d": dict(cls="libs.models.pino_models:FNO2d", args=[[6, 6, 6], [8, 8, 8]], kw=dict(layers=[32] * 4), x=(2, 12, 32, 3)),
    "pino fno2d padded": dict(cls="libs.models.pino_models:FNO2d", args=[[6, 6, 6], [8, 8, 8]],
                              kw=dict(layers=[32] * 4, pad_ratio=[0.0, 1.0]), x=(2, 16, 32, 3)),
    "pino fno2d relu": dict(cls="libs.models.pino_models:FNO2d", args=[[6, 6, 6], [8, 8, 8]], kw=dict(layers=[32] * 4, act="relu"),
                            x=(2, 12, 32, 3)),
    "pino fno2d mixed widths": dict(cls="libs.models.pino_models:FNO2d", args=[[6, 6, 6], [8, 8, 8]], kw=dict(layers=[32, 32, 64, 64]),
                                    x=(2, 12, 32, 3)),
    # the recurrent operator and the regressors
    "fourier layer fused": dict(cls="neuralop.models.rno:FourierLayer2d", args=[8, 8, 32], kw={}, x=(2, 32, 32, 32), grad_x=True),
    # not square: rno.SpectralConv2d refuses, and the block kernels, which would take this grid, must not be asked
    "fourier layer not square": dict(cls="neuralop.models.rno:FourierLayer2d", args=[8, 8, 32], kw={}, x=(2, 32, 16, 32), grad_x=True),
    "fourier layer 40 x 40": dict(cls="neuralop.models.rno:FourierLayer2d", args=[8, 8, 32], kw={}, x=(2, 32, 40, 40), grad_x=True),
    "regressor layer tail": dict(cls="neuralop.models.rno:SpectralConvWithFC", args=[32, 32, 8, 8], kw=dict(activation="relu"),
                                 x=(2, 32, 32, 32), grad_x=True),
    "regressor layer no_engine_tail": dict(cls="neuralop.models.rno:SpectralConvWithFC", args=[32, 32, 8, 8], kw=dict(activation="relu"),
                                           x=(2, 32, 32, 32), grad_x=True, attrs={"no_engine_tail": True}),
    "regressor layer width 16": dict(cls="neuralop.models.rno:SpectralConvWithFC", args=[16, 16, 8, 8], kw=dict(activation="relu"),
                                     x=(2, 32, 32, 16), grad_x=True),
    "regressor3d layer": dict(cls="neuralop.models.spectral_regressor:SpectralConvWithFC3d", args=[32, 32, 4, 4, 4], kw={},
                              x=(1, 8, 8, 16, 32), grad_x=True),
    "regressor3d layer width 16": dict(cls="neuralop.models.spectral_regressor:SpectralConvWithFC3d", args=[16, 16, 4, 4, 4], kw={},
                                       x=(1, 8, 8, 16, 16), grad_x=True),
    "rno2d": dict(cls="neuralop.models.rno:RNO2d", args=[12, 12, 32, 0], kw=dict(layer_num=1), x=(2, 1, 32, 32, 1)),
    "rno2d wide twin": dict(cls="neuralop.models.rno:RNO2d", args=[12, 12, 34, 0], kw=dict(layer_num=1), x=(2, 1, 32, 32, 1)),
    "rno2d no_width_padding": dict(cls="neuralop.models.rno:RNO2d", args=[12, 12, 34, 0], kw=dict(layer_num=1), x=(2, 1, 32, 32, 1),
                                   attrs={"no_width_padding": True}),
}


def bits(*tensors):
    """sha1 over the bit images of the tensors, in order (None counts as nothing)"""
    import torch
    h = hashlib.sha1()
    for t in tensors:
        if t is not None:
            t = t.detach()
            h.update((torch.view_as_real(t.resolve_conj()) if t.is_complex() else t).contiguous().cpu().numpy().tobytes())
    return h.hexdigest()[:16]


def run_case(name, case, dev):
    """one seeded forward + backward (loss = sum of squares) of a case on `dev` under the launch log
    -> (launch records, {"y" / "dx" / "grads": sha1 of the bits; grads = every parameter gradient in named_parameters order})"""
    import torch
    from pde_policylearning_amd import _lib
    mod, cname = case["cls"].split(":")
    torch.manual_seed(0)
    model = getattr(importlib.import_module("pde_policylearning_amd." + mod), cname)(*case["args"], **case["kw"]).to(dev)
    for m in model.modules():
        for k, v in case.get("attrs", {}).items():
            setattr(m, k, v)
    gen = torch.Generator(device="cpu").manual_seed(1234)
    x = torch.randn(case["x"], generator=gen).to(dev).requires_grad_(bool(case.get("grad_x")))
    inputs = (x, (torch.rand((case["x"][0], 1), generator=gen) * 100 + 100).to(dev)) if case.get("re") else (x,)
    if case.get("bucket"):
        from pde_policylearning_amd.trainer import FlatGradBucket
        FlatGradBucket(model.parameters(), direct_module=model).zero()
    torch.manual_seed(1)               # dropout masks
    with _lib.launch_log() as log:
        y = model(*inputs)
        y.square().sum().backward()
        torch.cuda.synchronize()
    return log.records, {"y": bits(y), "dx": bits(x.grad), "grads": bits(*[p.grad for p in model.parameters()])}


def expand(text):
    """the kernel names of an EXPECTED entry: `N*[ a b ]` stands for a b repeated N times"""
    out, opened = [], []
    for t in text.split():
        if t.endswith("*["):
            opened.append((int(t[:-2]), len(out)))
        elif t == "]":
            n, i = opened.pop()
            out.extend(out[i:] * (n - 1))
        else:
            out.append(t)
    return out


EXPECTED = {
    'planes chain': ('chain',
        'k_pw_fwd_lift 4*[ k_rowdft_chan k_axis_fwd k_axis_fwd k_pack_w k_mode_gemm k_axis_inv k_axis_inv k_rowidft_chan '
        'k_pw_fwd_block ] k_pw_fwd_block k_proj_fwd k_proj_bwd k_channel_sums k_reduce_jobs 4*[ k_block_bwd k_reduce_jobs '
        'k_rowdft_chan k_axis_fwd k_axis_fwd k_mode_gemm_dw k_unpack_dw k_mode_gemm k_axis_inv k_axis_inv k_rowidft_chan '
        '] k_block_bwd k_reduce_jobs k_lift_bwd k_reduce_jobs'),
    'planes fused loose rows': ('fused',
        'k_pw_fwd_lift k_pack_w 4*[ k_rowdft_chan k_axis_fwd k_axis_fwd k_mode_gemv k_axis_inv k_axis_inv k_pw_fwd_block '
        '] k_pw_fwd_block k_proj_fwd k_proj_bwd k_channel_sums k_reduce_jobs k_block_bwd k_reduce_jobs 4*[ k_rowdft_chan '
        'k_axis_fwd k_axis_fwd k_mode_outer_dw k_mode_gemv_t k_axis_inv k_axis_inv k_block_bwd ] k_reduce_jobs '
        'k_unpack_dw k_lift_bwd k_reduce_jobs'),
    'planes relu addend': ('addend',
        'k_pw_fwd_lift 4*[ k_rowdft_chan k_axis_fwd k_axis_fwd k_pack_w k_mode_gemm k_axis_inv k_axis_inv k_rowidft_chan '
        'k_pw_fwd_block ] 4*[ k_block_bwd k_reduce_jobs k_rowdft_chan k_axis_fwd k_axis_fwd k_mode_gemm_dw k_unpack_dw '
        'k_mode_gemm k_axis_inv k_axis_inv k_rowidft_chan ] k_lift_bwd k_reduce_jobs'),
    'planes mixed widths': ('addend',
        'k_pw_fwd_lift 2*[ k_rowdft_chan k_axis_fwd k_axis_fwd k_pack_w k_mode_gemm k_axis_inv k_axis_inv k_rowidft_chan '
        'k_pw_fwd_block k_rowdft_chan k_axis_fwd k_axis_fwd k_pack_w k_mode_gemm k_axis_inv k_axis_inv k_rowidft_chan ] '
        'k_pw_fwd_block k_pw_fwd_block k_proj_fwd k_proj_bwd k_channel_sums 2*[ k_reduce_jobs k_block_bwd ] k_reduce_jobs '
        '2*[ k_rowdft_chan k_axis_fwd k_axis_fwd k_mode_gemm_dw k_unpack_dw k_mode_gemm k_axis_inv k_axis_inv '
        'k_rowidft_chan k_block_bwd k_reduce_jobs k_rowdft_chan k_axis_fwd k_axis_fwd k_mode_gemm_dw k_unpack_dw '
        'k_mode_gemm k_axis_inv k_axis_inv k_rowidft_chan ] k_lift_bwd k_reduce_jobs'),
    'planes width 16': ('torch',
        '4*[ k_rowdft_chan k_axis_fwd k_axis_fwd k_pack_w k_mode_gemm k_axis_inv k_axis_inv k_rowidft_chan ] 4*[ '
        'k_rowdft_chan k_axis_fwd k_axis_fwd k_mode_gemm_dw k_unpack_dw k_mode_gemm k_axis_inv k_axis_inv k_rowidft_chan '
        ']'),
    'planes no_engine_tail': ('chain',
        'k_pw_fwd_lift 4*[ k_rowdft_chan k_axis_fwd k_axis_fwd k_pack_w k_mode_gemm k_axis_inv k_axis_inv k_rowidft_chan '
        'k_pw_fwd_block ] 4*[ k_rowdft_chan k_axis_fwd k_axis_fwd k_mode_gemm_dw k_unpack_dw k_mode_gemm k_axis_inv '
        'k_axis_inv k_rowidft_chan k_block_bwd k_reduce_jobs ] k_lift_bwd k_reduce_jobs'),
    'policy grad_x': ('chain',
        'k_pw_fwd_lift 4*[ k_rowdft_chan k_axis_fwd k_axis_fwd k_pack_w k_mode_gemm k_axis_inv k_axis_inv k_rowidft_chan '
        'k_pw_fwd_block ] k_pw_fwd_block k_proj_fwd k_pack_w1_x3 k_proj_bwd k_channel_sums k_reduce_jobs 4*[ k_block_bwd '
        'k_reduce_jobs k_rowdft_chan k_axis_fwd k_axis_fwd k_mode_gemm_dw k_unpack_dw k_mode_gemm k_axis_inv k_axis_inv '
        'k_rowidft_chan ] k_block_bwd k_reduce_jobs k_lift_dx k_lift_bwd k_reduce_jobs'),
    'observer2d per-sample': ('chain',
        'k_pw_fwd_lift k_pw_fwd_lift 4*[ k_rowdft_chan k_axis_fwd k_axis_fwd k_pack_w k_mode_gemm k_axis_inv k_axis_inv '
        'k_rowidft_chan k_pw_fwd_block ] k_pw_fwd_block k_pw_fwd_block k_proj_fwd k_pack_w1_x3 k_proj_bwd k_channel_sums '
        '2*[ k_reduce_jobs k_block_bwd ] 4*[ k_reduce_jobs k_rowdft_chan k_axis_fwd k_axis_fwd k_mode_gemm_dw k_unpack_dw '
        'k_mode_gemm k_axis_inv k_axis_inv k_rowidft_chan k_block_bwd ] 2*[ k_reduce_jobs k_lift_bwd ] k_reduce_jobs'),
    'observer2d per-sample padded': ('chain',
        'k_pw_fwd_lift k_pw_fwd_lift 4*[ k_rowdft_chan k_axis_fwd k_axis_fwd k_pack_w k_mode_gemm k_axis_inv k_axis_inv '
        'k_rowidft_chan k_pw_fwd_block ] k_pw_fwd_block k_pw_fwd_block k_proj_fwd k_pack_w1_x3 k_proj_bwd k_channel_sums '
        '2*[ k_reduce_jobs k_block_bwd ] 4*[ k_reduce_jobs k_rowdft_chan k_axis_fwd k_axis_fwd k_mode_gemm_dw k_unpack_dw '
        'k_mode_gemm k_axis_inv k_axis_inv k_rowidft_chan k_block_bwd ] 2*[ k_reduce_jobs k_lift_bwd ] k_reduce_jobs'),
    'observer2d grad_x': ('chain',
        'k_pw_fwd_lift 4*[ k_rowdft_chan k_axis_fwd k_axis_fwd k_pack_w k_mode_gemm k_axis_inv k_axis_inv k_rowidft_chan '
        'k_pw_fwd_block ] k_pw_fwd_block k_proj_fwd k_pack_w1_x3 k_proj_bwd k_channel_sums k_reduce_jobs 4*[ k_block_bwd '
        'k_reduce_jobs k_rowdft_chan k_axis_fwd k_axis_fwd k_mode_gemm_dw k_unpack_dw k_mode_gemm k_axis_inv k_axis_inv '
        'k_rowidft_chan ] k_block_bwd k_reduce_jobs k_lift_dx k_lift_bwd k_reduce_jobs'),
    'observer2d grad_x padded': ('chain',
        'k_pw_fwd_lift 4*[ k_rowdft_chan k_axis_fwd k_axis_fwd k_pack_w k_mode_gemm k_axis_inv k_axis_inv k_rowidft_chan '
        'k_pw_fwd_block ] k_pw_fwd_block k_proj_fwd k_pack_w1_x3 k_proj_bwd k_channel_sums k_reduce_jobs 4*[ k_block_bwd '
        'k_reduce_jobs k_rowdft_chan k_axis_fwd k_axis_fwd k_mode_gemm_dw k_unpack_dw k_mode_gemm k_axis_inv k_axis_inv '
        'k_rowidft_chan ] k_block_bwd k_reduce_jobs k_lift_dx k_lift_bwd k_reduce_jobs'),
    'fno2d whole model': ('',
        'k_pack_w k_lift_rowdft k_spec_mid k_pw_fwd_block0 3*[ k_spec_mid k_pw_fwd_block ] k_proj_fwd k_pack_w1_x3 '
        'k_proj_bwd k_channel_sums 4*[ k_spec_mid k_block_bwd ] k_lift_dx k_mode_gemm_dw k_reduce_jobs k_unpack_dw'),
    'fno2d width 16': ('torch',
        '4*[ k_rowdft_chan k_axis_fwd k_pack_w k_mode_gemm k_axis_inv k_rowidft_chan ] 4*[ k_channel_sums k_reduce_slabs '
        'k_rowdft_chan k_axis_fwd k_mode_gemm_dw k_unpack_dw k_mode_gemm k_axis_inv k_rowidft_chan ]'),
    'fno2d padded fused': ('fused',
        'k_pw_fwd_lift k_domain_pad k_pack_w k_rowdft_tile 4*[ k_spec_mid k_pw_fwd_block ] k_domain_crop k_proj_fwd '
        'k_pack_w1_x3 k_proj_bwd k_channel_sums k_reduce_jobs k_domain_pad k_rowdft_tile 4*[ k_spec_mid k_block_bwd ] '
        'k_mode_gemm_dw k_reduce_jobs k_unpack_dw k_domain_crop k_lift_dx k_lift_bwd k_reduce_jobs'),
    'fno2d padded per layer': ('torch',
        'k_pw_fwd_lift k_domain_pad 4*[ k_rowdft_chan k_axis_fwd k_pack_w k_mode_gemm k_axis_inv k_rowidft_chan ] '
        'k_domain_crop k_proj_fwd k_pack_w1_x3 k_proj_bwd k_channel_sums k_reduce_jobs k_domain_pad 4*[ k_channel_sums '
        'k_reduce_slabs k_rowdft_chan k_axis_fwd k_mode_gemm_dw k_unpack_dw k_mode_gemm k_axis_inv k_rowidft_chan ] '
        'k_domain_crop k_lift_dx k_lift_bwd k_reduce_jobs'),
    'fno2d mlp': ('fused fused fused fused',
        'k_pw_fwd_lift 4*[ k_pack_w k_rowdft_tile k_spec_mid k_pw_fwd_block k_cmlp_fwd ] k_proj_fwd k_pack_w1_x3 '
        'k_proj_bwd k_channel_sums k_reduce_jobs 4*[ k_cmlp_bwd k_reduce_jobs k_rowdft_tile k_spec_mid k_mode_gemm_dw '
        'k_block_bwd k_reduce_jobs k_unpack_dw ] k_lift_dx k_lift_bwd k_reduce_jobs'),
    'fno2d mlp padded': ('fused fused fused fused',
        'k_pw_fwd_lift k_domain_pad 4*[ k_pack_w k_rowdft_tile k_spec_mid k_pw_fwd_block k_cmlp_fwd ] k_domain_crop '
        'k_proj_fwd k_pack_w1_x3 k_proj_bwd k_channel_sums k_reduce_jobs k_domain_pad 4*[ k_cmlp_bwd k_reduce_jobs '
        'k_rowdft_tile k_spec_mid k_mode_gemm_dw k_block_bwd k_reduce_jobs k_unpack_dw ] k_domain_crop k_lift_bwd '
        'k_reduce_jobs'),
    'fno2d mlp composition': ('torch torch torch torch',
        'k_pw_fwd_lift 4*[ k_rowdft_chan k_axis_fwd k_pack_w k_mode_gemm k_axis_inv k_rowidft_chan k_cmlp_fwd ] '
        'k_proj_fwd k_pack_w1_x3 k_proj_bwd k_channel_sums k_reduce_jobs 4*[ k_cmlp_bwd k_reduce_jobs k_channel_sums '
        'k_reduce_slabs k_rowdft_chan k_axis_fwd k_mode_gemm_dw k_unpack_dw k_mode_gemm k_axis_inv k_rowidft_chan ] '
        'k_lift_bwd k_reduce_jobs'),
    'fno2d incremental direct': ('torch',
        '4*[ k_rowdft_tile k_axis_fwd k_pack_w k_mode_gemm k_axis_inv k_rowidft_tile ] 4*[ k_channel_sums k_reduce_slabs '
        'k_rowdft_tile k_axis_fwd k_mode_gemm_dw k_unpack_dw k_mode_gemm k_axis_inv k_rowidft_tile ]'),
    'fno2d direct': ('',
        'k_pack_w k_lift_rowdft k_spec_mid k_pw_fwd_block0 3*[ k_spec_mid k_pw_fwd_block ] k_proj_fwd k_pack_w1_x3 '
        'k_proj_bwd k_channel_sums 3*[ k_spec_mid k_block_bwd ] k_spec_mid k_block_bwd0 k_mode_gemm_dw k_reduce_jobs '
        'k_unpack_dw'),
    'fno3d': ('torch',
        '4*[ k_rowdft_chan k_axis_fwd k_axis_fwd k_pack_w k_mode_gemm k_axis_inv k_axis_inv k_rowidft_chan ] 4*[ '
        'k_channel_sums k_reduce_slabs k_rowdft_chan k_axis_fwd k_axis_fwd k_mode_gemm_dw k_unpack_dw k_mode_gemm '
        'k_axis_inv k_axis_inv k_rowidft_chan ]'),
    'fno3d padded': ('fused',
        'k_pw_fwd_lift k_domain_pad k_pack_w k_rowdft_tile 4*[ k_axis_fwd k_axis_fwd k_mode_gemm k_axis_inv k_axis_inv '
        'k_pw_fwd_block ] k_domain_crop k_proj_fwd k_pack_w1_x3 k_proj_bwd k_channel_sums k_reduce_jobs k_domain_pad '
        'k_rowdft_tile 4*[ k_axis_fwd k_axis_fwd k_mode_gemm k_axis_inv k_axis_inv k_block_bwd ] k_mode_gemm_dw '
        'k_reduce_jobs k_unpack_dw k_domain_crop k_lift_bwd k_reduce_jobs'),
    'fno1d': ('chain chain',
        'k_pw_fwd_lift 4*[ k_s1_ana k_s1_mix k_s1_syn k_pw_fwd_block ] k_proj_fwd k_pack_w1_x3 k_proj_bwd k_channel_sums '
        '4*[ k_reduce_jobs k_s1_ana k_s1_mix k_s1_syn k_block_bwd ] k_reduce_jobs k_lift_dx k_lift_bwd k_reduce_jobs'),
    'fno1d padded': ('chain chain',
        'k_pw_fwd_lift k_domain_pad 4*[ k_s1_ana k_s1_mix k_s1_syn k_pw_fwd_block ] k_domain_crop k_proj_fwd k_pack_w1_x3 '
        'k_proj_bwd k_channel_sums k_reduce_jobs k_domain_pad 4*[ k_s1_ana k_s1_mix k_s1_syn k_block_bwd k_reduce_jobs ] '
        'k_domain_crop k_lift_dx k_lift_bwd k_reduce_jobs'),
    'fno1d one layer': ('chain chain',
        'k_pw_fwd_lift k_s1_ana k_s1_mix k_s1_syn k_pw_fwd_block k_proj_fwd k_pack_w1_x3 k_proj_bwd k_channel_sums '
        'k_reduce_jobs k_s1_ana k_s1_mix k_s1_syn k_block_bwd k_reduce_jobs k_lift_bwd k_reduce_jobs'),
    'pino fno1d': ('chain chain',
        'k_pw_fwd_lift 3*[ k_s1_ana k_s1_mix k_s1_syn k_pw_fwd_block ] k_proj_fwd k_pack_w1_x3 k_proj_bwd k_channel_sums '
        '3*[ k_reduce_jobs k_s1_ana k_s1_mix k_s1_syn k_block_bwd ] k_reduce_jobs k_lift_bwd k_reduce_jobs'),
    'pino fno1d relu': ('torch torch',
        '6*[ k_s1_ana k_s1_mix k_s1_syn ]'),
    'pino fno1d fc_dim 64': ('torch torch',
        '6*[ k_s1_ana k_s1_mix k_s1_syn ]'),
    'pino fno2d': ('chain chain',
        'k_pw_fwd_lift k_rowdft_tile 2*[ k_axis_fwd k_pack_w k_mode_gemm k_axis_inv k_rowidft_tile k_pw_fwd_block '
        'k_rowdft_chan ] k_axis_fwd k_pack_w k_mode_gemm k_axis_inv k_rowidft_tile k_pw_fwd_block 3*[ k_rowdft_tile '
        'k_axis_fwd k_mode_gemm_dw k_unpack_dw k_mode_gemm k_axis_inv k_rowidft_tile k_block_bwd k_reduce_jobs ] '
        'k_lift_bwd k_reduce_jobs'),
    'pino fno2d padded': ('chain chain',
        'k_pw_fwd_lift k_rowdft_tile 2*[ k_axis_fwd k_pack_w k_mode_gemm k_axis_inv k_rowidft_tile k_pw_fwd_block '
        'k_rowdft_chan ] k_axis_fwd k_pack_w k_mode_gemm k_axis_inv k_rowidft_tile k_pw_fwd_block 3*[ k_rowdft_tile '
        'k_axis_fwd k_mode_gemm_dw k_unpack_dw k_mode_gemm k_axis_inv k_rowidft_tile k_block_bwd k_reduce_jobs ] '
        'k_lift_bwd k_reduce_jobs'),
    'pino fno2d relu': ('torch torch',
        '3*[ k_rowdft_tile k_axis_fwd k_pack_w k_mode_gemm k_axis_inv k_rowidft_tile ] 3*[ k_rowdft_tile k_axis_fwd '
        'k_mode_gemm_dw k_unpack_dw k_mode_gemm k_axis_inv k_rowidft_tile ]'),
    'pino fno2d mixed widths': ('torch torch',
        '3*[ k_rowdft_tile k_axis_fwd k_pack_w k_mode_gemm k_axis_inv k_rowidft_tile ] 3*[ k_rowdft_tile k_axis_fwd '
        'k_mode_gemm_dw k_unpack_dw k_mode_gemm k_axis_inv k_rowidft_tile ]'),
    'fourier layer fused': ('fused',
        'k_pack_w k_rowdft_tile k_spec_mid k_pw_fwd_block k_rowdft_tile k_spec_mid k_mode_gemm_dw k_block_bwd '
        'k_reduce_jobs k_unpack_dw'),
    'fourier layer not square': ('torch',
        'refused'),
    'fourier layer 40 x 40': ('torch',
        'k_rowdft_chan k_axis_fwd k_pack_w k_mode_gemm k_axis_inv k_rowidft_chan k_rowdft_chan k_axis_fwd k_mode_gemm_dw '
        'k_unpack_dw k_mode_gemm k_axis_inv k_rowidft_chan'),
    'regressor layer tail': ('',
        'k_pack_w k_rowdft_tile_drop k_spec_mid k_pw_fwd_block k_rowdft_tile_relu k_spec_mid k_mode_gemm_dw k_block_bwd '
        'k_reduce_jobs k_unpack_dw'),
    'regressor layer no_engine_tail': ('',
        'k_rowdft_tile k_axis_fwd k_pack_w k_mode_gemm k_axis_inv k_rowidft_tile k_pw_fwd_block k_block_bwd k_reduce_jobs '
        'k_rowdft_tile k_axis_fwd k_mode_gemm_dw k_unpack_dw k_mode_gemm k_axis_inv k_rowidft_tile'),
    'regressor layer width 16': ('',
        'k_rowdft_chan k_axis_fwd k_pack_w k_mode_gemm k_axis_inv k_rowidft_chan k_rowdft_chan k_axis_fwd k_mode_gemm_dw '
        'k_unpack_dw k_mode_gemm k_axis_inv k_rowidft_chan'),
    'regressor3d layer': ('',
        'k_rowdft_chan k_axis_fwd k_axis_fwd k_pack_w k_mode_gemm k_axis_inv k_axis_inv k_rowidft_chan k_pw_fwd_block '
        'k_block_bwd k_reduce_jobs k_rowdft_chan k_axis_fwd k_axis_fwd k_mode_gemm_dw k_unpack_dw k_mode_gemm k_axis_inv '
        'k_axis_inv k_rowidft_chan'),
    'regressor3d layer width 16': ('',
        'k_rowdft_chan k_axis_fwd k_axis_fwd k_pack_w k_mode_gemm k_axis_inv k_axis_inv k_rowidft_chan k_rowdft_chan '
        'k_axis_fwd k_axis_fwd k_mode_gemm_dw k_unpack_dw k_mode_gemm k_axis_inv k_axis_inv k_rowidft_chan'),
    'rno2d': ('fused',
        'k_pw_fwd_lift k_pack_w k_rowdft_tile k_axis_fwd_tlds k_mode_gemm k_axis_inv_tlds 4*[ k_pw_fwd_block ] k_pack_w '
        'k_rowdft_tile k_axis_fwd_tlds k_mode_gemm k_axis_inv_tlds 3*[ k_pw_fwd_block ] k_rno_reset_fwd k_pack_w '
        'k_rowdft_tile k_axis_fwd_tlds k_mode_gemm k_axis_inv_tlds k_pw_fwd_block k_rno_out_fwd 2*[ k_pack_w '
        'k_rowdft_tile_drop k_axis_fwd_tlds k_mode_gemm k_axis_inv_tlds k_pw_fwd_block ] 2*[ k_rowdft_tile_relu '
        'k_axis_fwd_tlds k_mode_gemm_dw k_mode_gemm k_axis_inv_tlds k_block_bwd k_reduce_jobs k_unpack_dw ] k_rno_out_bwd '
        'k_rowdft_tile k_axis_fwd_tlds k_mode_gemm_dw k_mode_gemm k_axis_inv_tlds k_block_bwd k_reduce_jobs k_unpack_dw '
        'k_rno_reset_bwd 3*[ k_rowdft_tile ] k_axis_fwd_tlds k_mode_gemm_dw k_mode_gemm k_axis_inv_tlds 3*[ k_block_bwd ] '
        'k_reduce_jobs k_unpack_dw 4*[ k_rowdft_tile ] k_axis_fwd_tlds k_mode_gemm_dw k_mode_gemm k_axis_inv_tlds 4*[ '
        'k_block_bwd ] k_reduce_jobs k_unpack_dw k_lift_bwd k_reduce_jobs'),
    'rno2d wide twin': ('fused',
        'k_pw_fwd_lift k_pack_w k_rowdft_tile k_axis_fwd_tlds k_mode_gemm k_axis_inv_tlds 4*[ k_pw_fwd_block ] k_pack_w '
        'k_rowdft_tile k_axis_fwd_tlds k_mode_gemm k_axis_inv_tlds 3*[ k_pw_fwd_block ] k_rno_reset_fwd k_pack_w '
        'k_rowdft_tile k_axis_fwd_tlds k_mode_gemm k_axis_inv_tlds k_pw_fwd_block k_rno_out_fwd 2*[ k_pack_w '
        'k_rowdft_tile_drop k_axis_fwd_tlds k_mode_gemm k_axis_inv_tlds k_pw_fwd_block ] k_proj_fwd k_pack_w1_x3 '
        'k_proj_bwd k_channel_sums k_reduce_jobs 2*[ k_rowdft_tile_relu k_axis_fwd_tlds k_mode_gemm_dw k_mode_gemm '
        'k_axis_inv_tlds k_block_bwd k_reduce_jobs k_unpack_dw ] k_rno_out_bwd k_rowdft_tile k_axis_fwd_tlds '
        'k_mode_gemm_dw k_mode_gemm k_axis_inv_tlds k_block_bwd k_reduce_jobs k_unpack_dw k_rno_reset_bwd 3*[ '
        'k_rowdft_tile ] k_axis_fwd_tlds k_mode_gemm_dw k_mode_gemm k_axis_inv_tlds 3*[ k_block_bwd ] k_reduce_jobs '
        'k_unpack_dw 4*[ k_rowdft_tile ] k_axis_fwd_tlds k_mode_gemm_dw k_mode_gemm k_axis_inv_tlds 4*[ k_block_bwd ] '
        'k_reduce_jobs k_unpack_dw k_lift_bwd k_reduce_jobs'),
    'rno2d no_width_padding': ('torch torch torch torch torch torch torch torch',
        '2*[ k_rowdft_chan k_axis_fwd_tlds k_pack_w k_mode_gemm k_axis_inv_tlds k_rowidft_chan ] k_rno_reset_fwd 6*[ '
        'k_rowdft_chan k_axis_fwd_tlds k_pack_w k_mode_gemm k_axis_inv_tlds k_rowidft_chan ] k_rno_out_fwd 2*[ '
        'k_rowdft_chan k_axis_fwd_tlds k_pack_w k_mode_gemm k_axis_inv_tlds k_rowidft_chan ] 2*[ k_rowdft_chan '
        'k_axis_fwd_tlds k_mode_gemm_dw k_unpack_dw k_mode_gemm k_axis_inv_tlds k_rowidft_chan ] k_rno_out_bwd 6*[ '
        'k_rowdft_chan k_axis_fwd_tlds k_mode_gemm_dw k_unpack_dw k_mode_gemm k_axis_inv_tlds k_rowidft_chan ] '
        'k_rno_reset_bwd 2*[ k_rowdft_chan k_axis_fwd_tlds k_mode_gemm_dw k_unpack_dw k_mode_gemm k_axis_inv_tlds '
        'k_rowidft_chan ]'),
}
