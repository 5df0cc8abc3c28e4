"""Why episodes end (include/bez_sim.h: BEZ_END_*, BezEpisodeTensor, BEZ_FLAG_REWARD_TERMS) without a GPU: the C header against abi.py,
the binding, a numpy restatement of the reward's termination tests and term split checked against the reference's golden vectors,
the env.debug.rewards mapping, and the PPO epoch row / observer tags."""
import json
import os
import re

import numpy as np

from bez_isaacgym_amd import abi
from tests.episode_stats_ref import GOLDEN_SETS, end_causes, golden_inputs, kick_params, task_params
from tests.fake_env import _CountingFakeEnv, _agent

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = open(os.path.join(ROOT, "include", "bez_sim.h")).read()
SIM_HIP = open(os.path.join(ROOT, "bez_isaacgym_amd", "csrc", "bez_sim.hip")).read()


# ---------------------------------------------------------------------------------------------------- the restatement (tests/episode_stats_ref.py)

def deciding(task, bits):
    return np.array([abi.end_cause(task, int(b)) for b in bits])


# ---------------------------------------------------------------------------------------------------- the contract
def _define(name, suffix=""):
    return int(re.search(r"#define %s (\d+)%s\b" % (name, suffix), HDR).group(1))


def test_header_constants_match_abi():
    assert _define("BEZ_FLAG_REWARD_TERMS", "u") == abi.FLAG_REWARD_TERMS == 16384
    for k, name in enumerate(["CARRIED", "FALL", "OUT_OF_BOUNDS", "OFF_COURSE", "GOAL", "TIMEOUT", "NONFINITE"]):
        assert _define("BEZ_END_" + name) == getattr(abi, "END_" + name) == k
    assert _define("BEZ_END_CAUSES") == abi.END_CAUSES == abi.REWARD_TERM_SLOTS == 8
    for name in ("END_BITS", "END_COUNTS", "REWARD_TERMS"):
        assert int(re.search(r"\bBEZ_EPISODE_%s = (\d+)," % name, HDR).group(1)) == getattr(abi, "EPISODE_" + name)
    assert int(re.search(r"\bBEZ_DTYPE_I32 = (\d+)", HDR).group(1)) == abi.DTYPE_I32
    # additive: the old tensor enum and the ABI version are unchanged, and the old regexes still see only the old lines
    assert re.findall(r"BEZ_TENSOR_COUNT = (\d+)", HDR) == ["17"] and abi.TENSOR_COUNT == 17
    assert int(re.search(r"#define BEZ_SIM_ABI_VERSION (\d+)", HDR).group(1)) == abi.ABI_VERSION == 5
    assert abi.FLAG_REWARD_TERMS & (abi.FLAG_CLEATS | abi.FLAG_BOX_ASSET) == 0
    assert not abi.default_config(16).flags & abi.FLAG_REWARD_TERMS
    body = SIM_HIP[SIM_HIP.index("int bez_sim_default_config("):]
    assert "BEZ_FLAG_REWARD_TERMS" not in body[:body.index("\n}\n")]


def test_episode_tensor_entry_point_declared_and_bound():
    sig = r"int bez_sim_get_episode_tensor\(BezSim\* %s, int which, void\*\* dev_ptr, int64_t shape\[3\], int\* ndim, int\* dtype\)"
    assert re.search(sig % "sim" + ";", HDR) and re.search(sig % "s", SIM_HIP)
    from bez_isaacgym_amd import sim
    assert "bez_sim_get_episode_tensor" in sim.EXPORTS
    assert '"bez_sim_get_episode_tensor": (C.c_int, [vp, C.c_int, C.POINTER(vp), C.POINTER(i64), C.POINTER(C.c_int), C.POINTER(C.c_int)])' \
        in open(sim.__file__).read()
    assert hasattr(sim.BezSim, "episode_tensor")


def test_deciding_cause_follows_the_reference_order():
    K, W, O = abi.TASK_KICK, abi.TASK_WALK, abi.TASK_ORIENT
    b = lambda *ks: sum(1 << k for k in ks)
    assert abi.end_cause(K, b(abi.END_FALL, abi.END_OFF_COURSE)) == abi.END_OFF_COURSE
    assert abi.end_cause(K, b(abi.END_GOAL, abi.END_OFF_COURSE)) == abi.END_GOAL
    assert abi.end_cause(W, b(abi.END_GOAL, abi.END_OFF_COURSE)) == abi.END_OFF_COURSE   # walk: heading after goal
    assert abi.end_cause(O, b(abi.END_GOAL, abi.END_OUT_OF_BOUNDS)) == abi.END_OUT_OF_BOUNDS
    assert abi.end_cause(O, b(abi.END_FALL, abi.END_GOAL)) == abi.END_GOAL
    for t in (K, W, O):
        assert abi.end_cause(t, b(abi.END_CARRIED)) == abi.END_CARRIED
        assert abi.end_cause(t, b(abi.END_CARRIED, abi.END_FALL)) == abi.END_FALL
        assert abi.end_cause(t, b(abi.END_TIMEOUT, abi.END_FALL, abi.END_CARRIED)) == abi.END_TIMEOUT
        assert abi.end_cause(t, b(abi.END_NONFINITE)) == abi.END_NONFINITE


# ---------------------------------------------------------------------------------------------------- the restatement vs the goldens
def test_restatement_reproduces_the_goldens():
    terminating = {}
    for task, tag in GOLDEN_SETS:
        t, x, prm, rew, rst = golden_inputs(task, tag)
        out = end_causes(t, x, prm)
        bits = out["bits"]
        np.testing.assert_array_equal(bits != 0, rst == 1, err_msg="%s %s: bits != 0 <=> rst" % (task, tag))
        ended = bits != 0
        # terminating rows: the deciding cause's reward rule (CARRIED alone: the shaping reward stands)
        np.testing.assert_allclose(out["rew"][ended], rew[ended], atol=3e-4, rtol=2e-5, err_msg="%s %s terminating" % (task, tag))
        # the other rows: the slots sum to the reward
        np.testing.assert_allclose(out["terms"][~ended].sum(1), rew[~ended], atol=1e-5, rtol=1e-5, err_msg="%s %s shaping" % (task, tag))
        terminating[(task, tag)] = int(ended.sum())
    assert terminating[("kick", "normal")] + terminating[("kick", "edge")] == 22, terminating
    # every cause a golden set can show shows up somewhere
    seen = set()
    for task, tag in GOLDEN_SETS:
        t, x, prm, _, _ = golden_inputs(task, tag)
        b = end_causes(t, x, prm)["bits"]
        seen |= {(task, k) for k in range(7) for v in b if v & (1 << k)}
    assert {("kick", k) for k in (0, 1, 2, 3, 4, 5)} <= seen, sorted(seen)


# ---------------------------------------------------------------------------------------------------- configuration
def _task_cfg(**env_extra):
    import yaml
    with open(os.path.join(ROOT, "bez_isaacgym_amd", "cfg", "task", "bez_kick.yaml")) as f:
        cfg = yaml.safe_load(f)
    cfg["env"]["numEnvs"] = 8
    cfg["env"].update(env_extra)
    return cfg


def test_debug_rewards_key_maps_to_the_flag():
    assert not abi.config_from_task_cfg(_task_cfg()).flags & abi.FLAG_REWARD_TERMS
    c = abi.config_from_task_cfg(_task_cfg(debug={"rewards": True}))
    assert c.flags & abi.FLAG_REWARD_TERMS
    assert c.flags & abi.FLAG_NONFINITE_GUARD and c.flags & abi.FLAG_IMU_PREV_ALIAS   # nothing else changes
    assert abi.config_from_task_cfg(_task_cfg(debug={"rewards": True})).flags & ~abi.FLAG_REWARD_TERMS == \
        abi.config_from_task_cfg(_task_cfg()).flags


# ---------------------------------------------------------------------------------------------------- PPO epoch row and observer


def test_epoch_row_carries_episode_ends():
    n, horizon = 32, 8
    env = _CountingFakeEnv(n, seed=7)
    env.episode_end_counts[2, 5] = 9   # counts from before the agent existed are not this agent's epochs
    agent = _agent(env, n, horizon)
    rows = [agent.train_epoch() for _ in range(3)]
    for k, row in enumerate(rows):
        ends = row["episode_ends"]
        assert set(ends) == set(abi.END_NAMES[:7])
        assert sum(ends.values()) == sum(env.ended[k * horizon:(k + 1) * horizon]) > 0, (k, ends)
        assert ends["carried"] == ends["nonfinite"] == ends["goal"] == 0
        assert "reward_terms" not in row
    assert sum(sum(r["episode_ends"].values()) for r in rows) == env.episode_end_counts.sum().item() - 9
    tot = {c: sum(r["episode_ends"][c] for r in rows) for c in ("fall", "out_of_bounds", "off_course")}
    assert tot == {c: env.episode_end_counts[getattr(abi, "END_" + c.upper())].sum().item() - (9 if c == "out_of_bounds" else 0)
                   for c in tot}


def test_epoch_row_carries_reward_terms_and_zeroes_them():
    n, horizon = 16, 8
    env = _CountingFakeEnv(n, seed=3, terms=True)
    agent = _agent(env, n, horizon)
    rewards = []
    orig = env.step

    def step(actions):
        out = orig(actions)
        rewards.append(out[1].sum().item())
        return out
    env.step = step
    rows = [agent.train_epoch() for _ in range(2)]
    for k, row in enumerate(rows):
        terms = row["reward_terms"]
        assert sorted(terms) == list(range(8))
        assert abs(sum(terms.values()) * n * horizon - sum(rewards[k * horizon:(k + 1) * horizon])) < 1e-3
        assert terms[1] == terms[3] == terms[4] == terms[6] == terms[7] == 0.0
    assert env.reward_terms_buf.abs().sum().item() == 0.0   # zeroed behind each epoch's read


def test_observer_writes_the_tags(tmp_path):
    from bez_isaacgym_amd.utils.rlgames_utils import RLGPUAlgoObserver
    obs = RLGPUAlgoObserver(str(tmp_path))
    obs.add(dict(epoch=1, frame=100, mean_reward=float("nan"), episode_ends=dict(fall=3, timeout=1, goal=0),
                 reward_terms={0: 0.5, 5: -0.25}))
    obs.add(dict(epoch=2, frame=200, mean_reward=float("nan"), episode_ends=dict(fall=0, timeout=0)))
    obs.f.close()
    rows = [json.loads(line) for line in open(os.path.join(str(tmp_path), "scalars.jsonl")).read().splitlines()]
    s = rows[0]["scalars"]
    assert s["episode_ends/fall"] == [0.75, 100] and s["episode_ends/timeout"] == [0.25, 100] and s["episode_ends/goal"] == [0.0, 100]
    assert s["rewards/0"] == [0.5, 100] and s["rewards/5"] == [-0.25, 100]
    assert rows[1]["scalars"]["episode_ends/fall"] == [0.0, 200] and "rewards/0" not in rows[1]["scalars"]
