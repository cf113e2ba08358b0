"""torch.autograd bridges onto the fnoengine C ABI: the only Python door into the engine.

PyTorch is plumbing here: it owns device memory (inputs, outputs, workspace, the
forward->backward stash) and the stream; all arithmetic happens in the HIP library.

One module per family; the families do not call each other, they share _core.py (all) and spectral.py (model, layers):
  _core      the operand check (_operand), the call (_call), the shape rules     every module imports it
  spectral   standalone spectral convolution, plan cache, corner weights, direct gradient writes
  model      fused FNO model, block stacks, RNO block tail, fan-out             (imports spectral)
  layers     RNO gates, pointwise convolutions, lifting, spectral + pointwise layer, projection head, channel MLP,
             domain padding                                                      (imports spectral)
  losses     relative Lp, PINO / Burgers / Darcy residual losses, Sobolev and Hs losses
  optim      fused Adam
  chanflow   3-D channel-flow solver (fp64)
  ctrl       closed-loop control: bridges, statistics, action and policy optimisers
  ns2d       2-D channel solver (fp64)
  data       device-resident training data

Callers write `from pde_policylearning_amd import functional as F` and read every name below from F.  The names are bound
here once, at import: module state (plan caches, DIRECT_WRITE_HOOKS, the single-use flags) lives in its home module and is
only ever mutated in place, so F.X and functional.<home>.X stay one object.  A stub assigned to F.X replaces what callers
outside the package see, not what a sibling inside it calls.
"""
import torch  # noqa: F401  (tests/hygiene.py swaps the `torch` and `_bytes` names of every module here, this one included)

from ._core import (
    _Tensor, _require_cuda, _bytes, _refuse, _operand, STREAM, _ptr, _call, _ptr_array, _plan_available, plane_size, gemm_mode,
    row_tiling, default_gelu_mask, _per_sample, _gpu_anchor)
from .spectral import (
    _spec_plans, _Cfg, _fill_params, _saved_params, spec_plan, DIRECT_WRITE_HOOKS, _SINGLE_USE, LAST_FORWARD_SINGLE_USE,
    single_use, plane_major, to_plane_major, _weights_ready, _check_corner_weights, _same_layout, _fresh_grads, _real_views,
    _direct_views, _notify_direct, _SpectralConvFn, spectral_conv)
from .model import (
    _model_plans, model_plan, model_plan_available, _ENDS, _FNOModelFn, fno_model, _block_tail, _FNOBlocksFn, blocks_supported,
    block_tail_supported, draw_dropout_seed, dropout_scale, fno_block_tail, fno_blocks, FANOUT_MAX, _FourierFanoutFn,
    fanout_supported, fourier_fanout)
from .layers import (
    gates_supported, _gate_operands, _RnoResetGateFn, _RnoOutputGateFn, rno_reset_gate, rno_output_gate, pointwise_supported,
    _PointwiseAddFn, pointwise_conv_add, _PointwisePerSampleFn, pointwise_conv_per_sample_bias, lifting_supported,
    _lifting_operands, _lifting_dx, _LiftingPerSampleFn, lifting_per_sample_bias, _LiftingFn, lifting, _ZeroLastPadsFn,
    zero_last_pads_, spectral_layer_supported, _SpectralLayerFn, spectral_pointwise_layer, PROJ_MAXCO, _ACT_CODES,
    projection_supported, _ProjectionHeadFn, projection_head, CHANNEL_MLP_WIDTHS, channel_mlp_supported, _ChannelMlpFn,
    channel_mlp, _domain_amounts, _domain_move, _domain_operand, _DomainPadFn, _DomainCropFn, domain_pad, domain_crop)
from .losses import (
    _LpLossRelFn, lp_loss_rel, _PinoLossFn, pino_loss, BURGERS_NX, _burgers_rows, burgers_loss_supported, _burgers_forward,
    _BurgersLossFn, burgers_loss, burgers_residual, DARCY_S_MIN, DARCY_S_MAX, _darcy_plane, darcy_loss_supported,
    _darcy_forward, _DarcyLossFn, darcy_loss, darcy_residual, SOBOLEV_REDUCE, sobolev_loss_supported, _sobolev_plan,
    _SobolevLossFn, sobolev_loss, HS_REDUCE, HS_GRIDS, HS_TERMS, hs_loss_supported, _hs_plan, _HsLossFn, hs_loss)
from .optim import (
    _adam_state, adam_step, adam_step_runs, adam_replay_scalars, adam_replay_dead)
from .chanflow import (
    ChannelGrid, chanflow_rhs, _ChanflowPdeLossFn, chanflow_pde_loss, CHANFLOW_DIAG, ChannelPoisson, chanflow_step_workspace,
    _chanflow_step_operands, chanflow_project, chanflow_wall_pressure, chanflow_rk3_step, chanflow_diagnostics,
    GraphedChannelStep, CONTROL_LOG, chanflow_diagnostics2_workspace, chanflow_diagnostics2)
from .ctrl import (
    STATS_MAX_FIELDS, _plane_stats, _strided_rows, ctrl_encode, ctrl_decode, running_stats_update, ACTION_PARTS, _action_rows,
    ctrl_action_begin, ctrl_action_workspace, ctrl_action_objective, ctrl_action_update, ctrl_action_finish, _policy_rows,
    ctrl_policy_begin, ctrl_policy_compose, ctrl_policy_unit_stats, ctrl_policy_objective, ctrl_policy_grad,
    GraphedControlLoop)
from .ns2d import (
    NS2D_SOLVE_OUT, NS2D_STATUS, NS2D_FIXED_OUT, NS2D_FIXED_STATUS, NS2D_DIAG, Ns2dGrid, _ns2d_operands, ns2d_solve,
    ns2d_fixed_mass, ns2d_diagnostics)
from .data import (
    _DATA_DTYPES, _data_indices, data_gather, _data_out, data_transpose_gather, pino_input)
