"""The DOF force tensor and actuator status (BEZ_FLAG_DOF_FORCE) without a GPU: the header against abi.py, the task key, the Python
argument / disabled-access errors, the recording translation units' resources against tests/golden/dof_force_kernel_resources.txt, and
the numpy restatement of the semantics (tests/dof_force_numpy.py) against an independent inverse dynamics on CPU-oracle steps."""
import concurrent.futures as cf
import os
import re

import numpy as np
import pytest
import torch

from bez_isaacgym_amd import abi
from tests.fake_env import _ActuatorFakeEnv, _agent

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "bez_sim.h")).read()
CSRC = os.path.join(ROOT, "bez_isaacgym_amd", "csrc")
RESOURCES = os.path.join(ROOT, "tests", "golden", "dof_force_kernel_resources.txt")
TUS = ("bez_step_ws8_df", "bez_step_ws8q_df", "bez_step_lane_df")


def _define(name):
    m = re.search(r"#define\s+%s\s+(\d+)u?\b" % name, HEADER)
    assert m, name
    return int(m.group(1))


def test_header_constants_match_the_binding():
    assert _define("BEZ_FLAG_DOF_FORCE") == abi.FLAG_DOF_FORCE == 32768
    for c, v in (("SATURATED_POS", abi.ACTUATOR_SATURATED_POS), ("SATURATED_NEG", abi.ACTUATOR_SATURATED_NEG),
                 ("LOCKED_POS", abi.ACTUATOR_LOCKED_POS), ("LOCKED_NEG", abi.ACTUATOR_LOCKED_NEG)):
        assert _define("BEZ_ACTUATOR_" + c) == v
    body = re.search(r"enum BezActuatorTensor \{(.*?)\};", HEADER, re.S).group(1)
    ids = dict((m.group(1), int(m.group(2))) for m in re.finditer(r"BEZ_ACTUATOR_(\w+) = (\d+)", body))
    assert ids == {"DOF_FORCE": abi.ACTUATOR_DOF_FORCE, "DRIVE_TORQUE": abi.ACTUATOR_DRIVE_TORQUE, "STATUS": abi.ACTUATOR_STATUS,
                   "TENSORS": abi.ACTUATOR_TENSORS}
    from bez_isaacgym_amd.sim import EXPORTS
    for fn in ("bez_sim_get_actuator_tensor", "bez_sim_refresh_actuator_tensors"):
        assert re.search(r"\bint %s\(" % fn, HEADER) and fn in EXPORTS


def test_abi_version_and_tensor_count_are_unchanged():
    assert _define("BEZ_SIM_ABI_VERSION") == abi.ABI_VERSION == 5
    assert re.search(r"BEZ_TENSOR_COUNT = 17\b", HEADER) and abi.TENSOR_COUNT == 17
    assert not abi.default_config(4).flags & abi.FLAG_DOF_FORCE   # off by default


def test_task_key_maps_to_the_flag_and_the_yamls_do_not_change():
    import yaml
    for task in ("bez_kick", "bez_walk", "bez_orient"):
        path = os.path.join(ROOT, "bez_isaacgym_amd", "cfg", "task", task + ".yaml")
        assert "enableDofForceSensors" not in open(path).read()
        cfg = yaml.safe_load(open(path))
        cfg["env"]["numEnvs"] = 8
        assert not abi.config_from_task_cfg(cfg, task=task).flags & abi.FLAG_DOF_FORCE
        cfg["env"]["enableDofForceSensors"] = True
        on = abi.config_from_task_cfg(cfg, task=task)
        assert on.flags & abi.FLAG_DOF_FORCE
        cfg["env"]["enableDofForceSensors"] = False
        assert abi.config_from_task_cfg(cfg, task=task).flags == on.flags & ~abi.FLAG_DOF_FORCE
        cfg["env"]["enableDofForceSensors"] = "yes"
        with pytest.raises(ValueError, match="enableDofForceSensors"):
            abi.config_from_task_cfg(cfg, task=task)


class _FakeLib:
    def __init__(self):
        self.calls = []

    def bez_sim_refresh_actuator_tensors(self, h, stream):
        self.calls.append("refresh")
        return 0

    def bez_sim_set_flags(self, h, flags):
        self.calls.append(("flags", flags))
        return 0


def _bare_sim(flags):
    from bez_isaacgym_amd.sim import BezSim
    s = BezSim.__new__(BezSim)
    s.cfg = abi.default_config(4); s.cfg.flags = flags
    s.lib, s.h, s.num_envs, s.device, s._views = _FakeLib(), None, 4, torch.device("cpu"), {}
    s._stream = lambda: None
    return s


def test_python_argument_and_disabled_access_errors():
    from bez_isaacgym_amd.sim import BezSimError
    off = _bare_sim(abi.FLAG_IMU_PREV_ALIAS)
    for call in (lambda: off.actuator_tensor(abi.ACTUATOR_DOF_FORCE), off.refresh_actuator_tensors):
        with pytest.raises(BezSimError, match="enableDofForceSensors"):
            call()
    assert off.lib.calls == []
    for bad in (3, -1, True, 1.0, "torque"):
        with pytest.raises(ValueError):
            off.actuator_tensor(bad)
    assert [abi.actuator_tensor_id(k) for k in ("dof_force", "Drive_Torque", " status ", 2)] == [0, 1, 2, 2]
    on = _bare_sim(abi.FLAG_IMU_PREV_ALIAS | abi.FLAG_DOF_FORCE)
    on.refresh_actuator_tensors()
    assert on.lib.calls == ["refresh"]
    off.set_flags(abi.FLAG_DOF_FORCE)          # toggled after creation: the binding follows
    off.refresh_actuator_tensors()
    assert off.lib.calls[-1] == "refresh"


def test_vec_task_attributes_exist_only_with_the_key():
    from bez_isaacgym_amd.tasks.base.vec_task import VecTask

    class _T(VecTask):
        def pre_physics_step(self, actions): pass
        def post_physics_step(self): pass
    t = _T.__new__(_T)
    for name in ("dof_force_tensor", "dof_drive_torque", "dof_status"):
        with pytest.raises(AttributeError, match="enableDofForceSensors"):
            getattr(t, name)
    with pytest.raises(AttributeError, match="enableDofForceSensors"):
        t.refresh_dof_force_tensor()
    with pytest.raises(AttributeError, match="no attribute"):
        t.some_other_name
    calls = []

    class _S:
        def refresh_actuator_tensors(self): calls.append(1)
    t._dof_force_views = ("net", "drive", "status"); t.sim = _S()
    assert t.refresh_dof_force_tensor() is True and calls == [1]
    assert (t.dof_force_tensor, t.dof_drive_torque, t.dof_status) == ("net", "drive", "status")


# ---- PPO epoch row and observer (tests/fake_env.py)


def test_epoch_row_gains_actuators_only_with_the_flag():
    from tests.fake_env import FakeVecEnv

    class _On(_ActuatorFakeEnv, FakeVecEnv):
        pass
    n = 16
    off = _agent(FakeVecEnv(n, seed=7), n, 8)
    rows_off = [off.train_epoch() for _ in range(2)]
    env = _On(n, seed=7)
    on = _agent(env, n, 8)
    rows_on = [on.train_epoch() for _ in range(2)]
    assert all("actuators" not in r for r in rows_off)
    assert all(set(r) == set(rows_off[0]) | {"actuators"} for r in rows_on)
    assert env.snapshots == 2                                  # one refresh per epoch
    a = rows_on[1]["actuators"]
    assert set(a) == set(on.ACTUATOR_NAMES)
    assert abs(a["mean_abs_drive_torque"] - 4.0 / 16) < 1e-12 and abs(a["saturated_share"] - 1.0 / 16) < 1e-12
    assert abs(a["locked_share"] - 0.5 / 16) < 1e-12 and abs(a["mean_positive_power"] - 5.0 / 16) < 1e-12
    # the rest of the row does not depend on the flag
    for r0, r1 in zip(rows_off, rows_on):
        for k in ("kl", "a_loss", "c_loss", "lr"):
            assert r0[k] == r1[k], k


def test_observer_writes_the_actuator_tags(tmp_path):
    import json
    from bez_isaacgym_amd.utils.rlgames_utils import RLGPUAlgoObserver
    ob = RLGPUAlgoObserver(str(tmp_path))
    ob.add(dict(epoch=1, frame=100, mean_reward=float("nan"), actuators=dict(mean_abs_drive_torque=0.5, saturated_share=0.25)))
    ob.add(dict(epoch=2, frame=200, mean_reward=float("nan")))
    ob.f.close()
    lines = open(os.path.join(str(tmp_path), "scalars.jsonl")).read().splitlines()
    s0 = json.loads(lines[0])["scalars"]
    assert s0["actuators/mean_abs_drive_torque"] == [0.5, 100] and s0["actuators/saturated_share"] == [0.25, 100]
    assert not any(k.startswith("actuators/") for k in json.loads(lines[1]).get("scalars", {}))


# ---- the recording translation units
@pytest.fixture(scope="module")
def resources(tmp_path_factory):
    from tests.kernel_resources import kernel_resources
    d = tmp_path_factory.mktemp("dfres")
    with cf.ThreadPoolExecutor(len(TUS)) as ex:
        res = list(ex.map(lambda tu: kernel_resources(os.path.join(CSRC, tu + ".hip"), str(d)), TUS))
    return dict(zip(TUS, res))


def test_recording_units_build_for_gfx950_with_the_recorded_resources(resources):
    """(vgpr, vgpr spills, sgpr, sgpr spills, scratch bytes, LDS bytes) of every instantiation = the committed table, so later changes show;
    every symbol carries a name of its own (no clash with the kernels a sim without the flag launches)."""
    want = {}
    for line in open(RESOURCES):
        if line.strip() and not line.startswith("#"):
            tu, name, *vals = line.split()
            want[(tu, name)] = tuple(int(v) for v in vals)
    got = {(tu, k): v for tu in TUS for k, v in resources[tu].items()}
    assert set(got) == set(want), set(got) ^ set(want)
    for tu in TUS:
        assert len(resources[tu]) == 10 and all("_df" in k and k.endswith("ParamsDFE") for k in resources[tu]), sorted(resources[tu])
    for key in want:
        assert got[key] == want[key], (key, got[key], want[key])


# ---- the semantics against an independent inverse dynamics, on the CPU oracle
@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_restated_net_joint_force_is_the_inverse_dynamics_torque(model, precision):
    """One substep (substeps = 1) of the oracle in free space without leg <-> leg contact, from 64 pressed states with the hip rolls at the
    default pose: on every joint that ends the substep off the speed limit and whose restated PD torque is inside 0.8 x effort, the restated
    tau_net equals rnea_floating's joint torque plus armature * qdd.  Bar 1e-5 N m (measured: 2.9e-7 on the fp64 oracle, 2.5e-6 on its fp32
    build, both from the fp32 read-back of the states); the subset is at least half the joint samples."""
    from tests import dof_force_numpy as D
    from tests import rbd_numpy as R
    from tests.scenarios import make_backend
    from tests.scenarios import _free_space_cfg, _pressed_state
    n = 64
    cfg = _free_space_cfg(n, substeps=1)
    cfg.flags |= abi.FLAG_NO_SELF_COLLISION
    sim = make_backend("oracle", cfg, precision=precision)
    sim.step(np.zeros((n, 18), np.float32))
    acts = D.inject_pressed(sim, n, model, 21, _pressed_state)
    rs0 = sim.root_states.reshape(n, 2, 13).astype(np.float64); ds0 = sim.dof_state.reshape(n, 18, 2).astype(np.float64)
    sim.pre_physics(acts); sim.simulate()
    rs1 = sim.root_states.reshape(n, 2, 13).astype(np.float64); ds1 = sim.dof_state.reshape(n, 18, 2).astype(np.float64)
    target = sim.targets.reshape(n, 18).astype(np.float64)
    tau, qdd = D.rnea_torques(R, model, cfg, rs0, rs1, ds0, ds1)
    pd, net, _ = D.restate(cfg, model, ds0[:, :, 0], ds0[:, :, 1], ds1[:, :, 0], ds1[:, :, 1], target)
    ok = D.easy_subset(cfg, pd, ds1[:, :, 1])
    err = np.abs(net - (tau + float(cfg.armature) * qdd))[ok]
    print("subset %d of %d, worst %.3g N m (%s)" % (ok.sum(), ok.size, err.max(), precision))
    assert ok.sum() >= ok.size // 2, ok.sum()
    assert err.max() < 1e-5, err.max()
