"""Host side of the control loop (no GPU): the run plan from base_control.yaml-style keys, the collector's writer against the
three dataset classes, the explosion check on a fabricated log, and the refusals that need no device."""
import argparse
import os

import numpy as np
import pytest
import torch

# key / value content in the style of the reference's configs/base_control.yaml (settings data, comments dropped)
BASE_CONTROL = """
project_name: control_v2
load_model_name: planes_channel180_minchan_28-RNO-reproduce.pth
exp_name: 10-RNO
display_variables:
  - exp_name
  - policy_name
DATA_FOLDER: ./data/planes_channel180_minchan
path_name: planes_channel180_minchan
model_name: FNO2dObserver
state_path_name: ./data/channel180_minchan.mat
use_v_plane: false
modes: 12
width: 32
vis_sample_img: false
control_timestep: 200
model_timestep: 1
noise_scale: 0.0
downsample_rate: 1
x_range: 32
y_range: 32
policy_name: gt
rand_scale: 1
collect_data: true
dump_state: false
detect_plane: -10
test_plane: -25
vis_frame: 60
vis_interval: 1000
output_dir: ./outputs
close_wandb: false
"""


def _plan(text, argv=()):
    import yaml
    from pde_policylearning_amd import run_control as RC
    return RC.plan_from_yaml(RC.build_parser().parse_args(list(argv)), yaml.safe_load(text))


def test_run_plan_from_control_yaml():
    plan = _plan(BASE_CONTROL, ["--ensemble", "4", "--graph"])
    assert plan.policy_name == "gt" and plan.steps == 201 and plan.detect_plane == -10 and plan.modes == 12 and plan.width == 32
    assert plan.collect_data is True and plan.collect_folder == os.path.join("./outputs", "10-RNO")
    assert plan.ensemble == 4 and plan.graph is True and plan.state_path_name == "./data/channel180_minchan.mat"
    assert plan.vis_frame == 60 and plan.close_wandb is False            # carried, ignored
    fno = _plan(BASE_CONTROL.replace("policy_name: gt", "policy_name: fno"))
    assert fno.collect_data is False and fno.collect_folder is None      # only gt / unmanipulated runs collect
    with pytest.raises(ValueError, match="initial condition"):
        _plan(BASE_CONTROL.replace("state_path_name: ./data/channel180_minchan.mat", "state_path_name:"))
    assert _plan(BASE_CONTROL.replace("state_path_name: ./data/channel180_minchan.mat", "state_path_name:"), ["--tanh-channel"]).tanh_channel


@pytest.mark.parametrize("name", ["rand", "optimal-observer", "optimal-policy-observer"])
def test_out_of_scope_policies_raise(name):
    from pde_policylearning_amd.control import make_policy
    with pytest.raises(NotImplementedError):
        make_policy(name)
    with pytest.raises(NotImplementedError):
        _plan(BASE_CONTROL.replace("policy_name: gt", f"policy_name: {name}"))
    with pytest.raises(RuntimeError, match="Not supported policy name"):
        make_policy("nonsense")


def test_control_loop_has_no_cpu_path():
    from pde_policylearning_amd.control import ControlLoop, GtPolicy

    class Env:
        device, B, Nx, Nz = "cpu", 1, 4, 4
    with pytest.raises(RuntimeError, match="no CPU path"):
        ControlLoop(Env(), GtPolicy(), 3)


def test_explosion_check_names_iteration_and_environment():
    from pde_policylearning_amd.control import check_log, infos_from_log
    from pde_policylearning_amd.libs.envs.control_env import ChannelFlowEnv
    log = np.ones((7, 3, 13))
    log[..., 0] = 0.0
    log[..., 12] = 3e-3
    check_log(log)
    log[5, 1, 0] = -10.5
    log[6, 0, 0] = 99.0
    with pytest.raises(RuntimeError, match=r"Control exploded! iteration 5, environment 1"):
        check_log(log)
    with pytest.raises(RuntimeError, match=r"iteration 5, environment 1"):
        check_log(log[4:], first=4)
    check_log(log[:5])
    log[2, 2, 0] = np.nan
    with pytest.raises(RuntimeError, match=r"iteration 2, environment 2"):
        check_log(log)
    infos = infos_from_log(log[:2], ChannelFlowEnv.INFO_KEYS, init=infos_from_log(log[:1], ChannelFlowEnv.INFO_KEYS)[0])
    assert len(infos) == 2 and len(infos[0]) == 3
    assert infos[1][0]["drag_reduction/3_3_dPdx_reverse_cal"] == 3e-3
    assert infos[1][0]["drag_reduction_relative/3_3_dPdx_reverse_cal"] == 1.0
    assert not any("divergence" in k for k in infos[1][0] if k.startswith("drag_reduction_relative"))


def test_writer_output_opens_with_the_dataset_classes(tmp_path):
    from pde_policylearning_amd.control import FIELDS, write_metadata, write_step
    from pde_policylearning_amd.libs.pde_data_loader import FullFieldNSDataset, PDEDataset, SequentialPDEDataset
    rng = np.random.default_rng(0)
    Nx, Ny, Nz, n = 8, 6, 8, 4
    shapes = {"P_planes": (Nx, Nz), "V_planes": (Nx, Nz), "U_field": (Nx, Ny + 1, Nz), "V_field": (Nx, Ny, Nz),
              "W_field": (Nx, Ny + 1, Nz), "du_dt": (Nx, Ny + 1, Nz)}
    folder = str(tmp_path)
    steps = [{k: 0.1 + rng.standard_normal(s) for k, s in shapes.items()} for _ in range(n)]
    for i, arrays in enumerate(steps):
        write_step(folder, i + 1, arrays)
    stats = {k: (np.stack([s[k] for s in steps]).mean(0), np.stack([s[k] for s in steps]).std(0)) for k in FIELDS}
    dpdx = 3e-3 + 1e-4 * np.arange(n)
    write_metadata(folder, 180.0, stats, dpdx)
    assert sorted(os.listdir(folder)) == sorted(["metadata.npy"] + [f"{k}_{str(i + 1).zfill(6)}.npy" for k in FIELDS for i in range(n)])
    args = argparse.Namespace(model_timestep=2)
    p, v = PDEDataset(args, folder, list(range(n)), 1, Nx, Nz)[2]
    want = (steps[2]["P_planes"] - stats["P_planes"][0]) / (stats["P_planes"][1] + 1e-5)
    assert tuple(p.shape) == (Nx, Nz, 1) and np.allclose(p[..., 0].numpy(), want, rtol=0, atol=1e-12)
    ps, vs = SequentialPDEDataset(args, folder, list(range(n)), 1, Nx, Nz)[1]
    assert tuple(ps.shape) == (2, Nx, Nz) and tuple(vs.shape) == (2, Nx, Nz)
    item = FullFieldNSDataset(args, folder, list(range(n)), [1, -2], 1, Nx, Nz)[1]
    assert tuple(item[2].shape) == (2, Nx, Ny + 1, Nz) and tuple(item[1].shape) == (2, 2, Nx, Nz)
    assert item[6].tolist() == [dpdx[2], dpdx[3]] and float(item[5][0]) == 180.0
    assert np.array_equal(item[3][0].numpy(), steps[2]["V_field"])
