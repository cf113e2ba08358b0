"""The surface of pde_policylearning_amd.functional, frozen when the module became a package: every name the single-file
module bound (dir() of it, without dunders and imported modules) still resolves on the package, module state is one object
however it is reached, and the package imports in a fresh interpreter (no cycle among its modules).  No GPU is needed."""
import importlib
import os
import subprocess
import sys

import pytest

from pde_policylearning_amd import functional as F

NAMES = """
    ACTION_PARTS BURGERS_NX CHANFLOW_DIAG CHANNEL_MLP_WIDTHS CONTROL_LOG ChannelGrid ChannelPoisson DARCY_S_MAX DARCY_S_MIN
    DIRECT_WRITE_HOOKS FANOUT_MAX GraphedChannelStep GraphedControlLoop HS_GRIDS HS_REDUCE HS_TERMS LAST_FORWARD_SINGLE_USE
    NS2D_DIAG NS2D_FIXED_OUT NS2D_FIXED_STATUS NS2D_SOLVE_OUT NS2D_STATUS Ns2dGrid PROJ_MAXCO SOBOLEV_REDUCE STATS_MAX_FIELDS
    STREAM _ACT_CODES _BurgersLossFn _Cfg _ChanflowPdeLossFn _ChannelMlpFn _DATA_DTYPES _DarcyLossFn _DomainCropFn _DomainPadFn
    _ENDS _FNOBlocksFn _FNOModelFn _FourierFanoutFn _HsLossFn _LiftingFn _LiftingPerSampleFn _LpLossRelFn _PinoLossFn
    _PointwiseAddFn _PointwisePerSampleFn _ProjectionHeadFn _RnoOutputGateFn _RnoResetGateFn _SINGLE_USE _SobolevLossFn
    _SpectralConvFn _SpectralLayerFn _Tensor _ZeroLastPadsFn _action_rows _adam_state _block_tail _burgers_forward _burgers_rows
    _bytes _call _chanflow_step_operands _check_corner_weights _darcy_forward _darcy_plane _data_indices _data_out _direct_views
    _domain_amounts _domain_move _domain_operand _fill_params _fresh_grads _gate_operands _gpu_anchor _hs_plan _lifting_dx
    _lifting_operands _model_plans _notify_direct _ns2d_operands _operand _per_sample _plan_available _plane_stats _policy_rows
    _ptr _ptr_array _real_views _refuse _require_cuda _same_layout _saved_params _sobolev_plan _spec_plans _strided_rows
    _weights_ready adam_replay_dead adam_replay_scalars adam_step adam_step_runs block_tail_supported blocks_supported
    burgers_loss burgers_loss_supported burgers_residual chanflow_diagnostics chanflow_diagnostics2
    chanflow_diagnostics2_workspace chanflow_pde_loss chanflow_project chanflow_rhs chanflow_rk3_step chanflow_step_workspace
    chanflow_wall_pressure channel_mlp channel_mlp_supported ctrl_action_begin ctrl_action_finish ctrl_action_objective
    ctrl_action_update ctrl_action_workspace ctrl_decode ctrl_encode ctrl_policy_begin ctrl_policy_compose ctrl_policy_grad
    ctrl_policy_objective ctrl_policy_unit_stats darcy_loss darcy_loss_supported darcy_residual data_gather
    data_transpose_gather default_gelu_mask domain_crop domain_pad draw_dropout_seed dropout_scale fanout_supported
    fno_block_tail fno_blocks fno_model fourier_fanout gates_supported gemm_mode hs_loss hs_loss_supported lifting
    lifting_per_sample_bias lifting_supported lp_loss_rel model_plan model_plan_available ns2d_diagnostics ns2d_fixed_mass
    ns2d_solve pino_input pino_loss plane_major plane_size pointwise_conv_add pointwise_conv_per_sample_bias pointwise_supported
    projection_head projection_supported rno_output_gate rno_reset_gate row_tiling running_stats_update single_use sobolev_loss
    sobolev_loss_supported spec_plan spectral_conv spectral_layer_supported spectral_pointwise_layer to_plane_major
    zero_last_pads_
""".split()

# module state and its one home: mutated in place there, never rebound (a second binding would fork it)
STATE = {"_spec_plans": "spectral", "DIRECT_WRITE_HOOKS": "spectral", "_SINGLE_USE": "spectral", "LAST_FORWARD_SINGLE_USE": "spectral",
         "_model_plans": "model", "_sobolev_plan": "losses", "_hs_plan": "losses"}


def test_the_list_is_the_single_file_modules():
    assert len(NAMES) == 181 and len(set(NAMES)) == 181 and NAMES == sorted(NAMES)


def test_every_name_resolves_on_the_package():
    assert [n for n in NAMES if not hasattr(F, n)] == []


@pytest.mark.parametrize("name,home", sorted(STATE.items()))
def test_state_is_one_object(name, home):
    owner = importlib.import_module(f"{F.__name__}.{home}")
    assert getattr(F, name) is getattr(owner, name)
    for mod in (m for n, m in sorted(sys.modules.items()) if n.startswith(F.__name__ + ".")):
        if name in mod.__dict__:
            assert mod.__dict__[name] is getattr(owner, name), mod.__name__


def test_single_use_reaches_the_state_callers_read():
    """the context manager writes where trainer.py reads (F.LAST_FORWARD_SINGLE_USE[0]) and where _direct_views reads"""
    was = F.LAST_FORWARD_SINGLE_USE[0]
    try:
        with F.single_use(False):
            assert F._SINGLE_USE[-1] is False and F.LAST_FORWARD_SINGLE_USE[0] is False
        assert F._SINGLE_USE == [True]
    finally:
        F.LAST_FORWARD_SINGLE_USE[0] = was


def test_imports_in_a_fresh_interpreter():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", "import pde_policylearning_amd.functional"], cwd=root, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
