"""The per-env non-finite guard (BEZ_FLAG_NONFINITE_GUARD) without a GPU: the C header against abi.py, the binding, the default /
task-config flag, and the PPO epoch row's nonfinite_resets."""
import os
import re

from bez_isaacgym_amd import abi
from tests.fake_env import FakeVecEnv, _GuardedFakeEnv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = open(os.path.join(ROOT, "include", "bez_sim.h")).read()
SIM_HIP = open(os.path.join(ROOT, "bez_isaacgym_amd", "csrc", "bez_sim.hip")).read()


def _define(name):
    return int(re.search(r"#define %s (\d+)u" % name, HDR).group(1))


def _enum(name):
    return int(re.search(r"\b%s = (\d+)," % name, HDR).group(1))


def test_header_constants_match_abi():
    assert _define("BEZ_FLAG_NONFINITE_GUARD") == abi.FLAG_NONFINITE_GUARD == 8192
    assert _define("BEZ_HEALTH_NONFINITE") == abi.HEALTH_NONFINITE == 1
    assert _define("BEZ_HEALTH_SPIN_TIMEOUT") == abi.HEALTH_SPIN_TIMEOUT == 2
    assert _enum("BEZ_TENSOR_NONFINITE_COUNT") == abi.TENSOR_NONFINITE_COUNT == 15
    assert _enum("BEZ_TENSOR_HEALTH") == abi.TENSOR_HEALTH == 16
    assert int(re.search(r"BEZ_TENSOR_COUNT = (\d+)", HDR).group(1)) == abi.TENSOR_COUNT == 17
    assert int(re.search(r"#define BEZ_SIM_ABI_VERSION (\d+)", HDR).group(1)) == abi.ABI_VERSION == 5   # additive: the config is unchanged
    # the new bit is no asset bit: bez_sim_set_flags may toggle it
    assert abi.FLAG_NONFINITE_GUARD & (abi.FLAG_CLEATS | abi.FLAG_BOX_ASSET) == 0


def test_health_entry_point_declared_and_bound():
    assert re.search(r"int bez_sim_health\(BezSim\* sim, uint64_t\* bits, int32_t clear, void\* stream\);", HDR)
    assert re.search(r"int bez_sim_health\(BezSim\* s, uint64_t\* bits, int32_t clear, void\* stream_\)", SIM_HIP)
    from bez_isaacgym_amd import sim
    assert "bez_sim_health" in sim.EXPORTS
    src = open(sim.__file__).read()
    assert '"bez_sim_health": (C.c_int, [vp, C.POINTER(u64), i32, vp])' in src
    assert hasattr(sim.BezSim, "health") and hasattr(sim.BezSim, "nonfinite_counts")


def test_default_config_has_the_guard_on_both_sides():
    assert abi.default_config(16).flags & abi.FLAG_NONFINITE_GUARD
    body = SIM_HIP[SIM_HIP.index("int bez_sim_default_config("):]
    body = body[:body.index("\n}\n")]
    assert re.search(r"c->flags = [^;]*BEZ_FLAG_NONFINITE_GUARD", body)


def _task_cfg(**env_extra):
    import yaml
    with open(os.path.join(ROOT, "bez_isaacgym_amd", "cfg", "task", "bez_kick.yaml")) as f:
        cfg = yaml.safe_load(f)
    cfg["env"]["numEnvs"] = 8
    cfg["env"].update(env_extra)
    return cfg


def test_task_config_honours_nonfinite_guard_key():
    assert abi.config_from_task_cfg(_task_cfg()).flags & abi.FLAG_NONFINITE_GUARD
    assert abi.config_from_task_cfg(_task_cfg(nonfiniteGuard=True)).flags & abi.FLAG_NONFINITE_GUARD
    c = abi.config_from_task_cfg(_task_cfg(nonfiniteGuard=False))
    assert not c.flags & abi.FLAG_NONFINITE_GUARD
    assert c.flags & abi.FLAG_IMU_PREV_ALIAS   # nothing else changes


def test_epoch_row_carries_nonfinite_resets():
    from bez_isaacgym_amd.ppo.a2c_continuous import A2CAgent
    from tests.fake_env import _params
    horizon = 8
    # epoch 0: none; epoch 1: env 3 twice and env 5 once (3 increments); epoch 2: env 0 once
    env = _GuardedFakeEnv(32, seed=7, trips={horizon + 2: {3: 1}, horizon + 5: {3: 1, 5: 1}, 2 * horizon: {0: 1}})
    env.nonfinite_buf[7] = 4   # counts from before the agent existed are not this agent's epochs
    agent = A2CAgent(_params(32, 128, horizon=horizon), env, "cpu")
    agent.obs = agent.env_reset()
    rows = [agent.train_epoch() for _ in range(3)]
    assert [r["nonfinite_resets"] for r in rows] == [0, 3, 1]
    assert all(r["sim_health"] == 0 for r in rows)


def test_epoch_row_without_counters_reports_zero():
    from bez_isaacgym_amd.ppo.a2c_continuous import A2CAgent
    from tests.fake_env import _params
    agent = A2CAgent(_params(16, 64, horizon=4), FakeVecEnv(16, seed=2), "cpu")
    agent.obs = agent.env_reset()
    row = agent.train_epoch()
    assert row["nonfinite_resets"] == 0 and row["sim_health"] == 0


def test_scalars_log_carries_the_tag(tmp_path):
    import json
    from bez_isaacgym_amd.utils.rlgames_utils import RLGPUAlgoObserver
    obs = RLGPUAlgoObserver(str(tmp_path))
    obs.add(dict(epoch=1, frame=100, mean_reward=float("nan"), nonfinite_resets=2))
    obs.f.close()
    row = json.loads(open(os.path.join(str(tmp_path), "scalars.jsonl")).read().splitlines()[-1])
    assert row["scalars"]["env/nonfinite_resets"] == [2, 100]
