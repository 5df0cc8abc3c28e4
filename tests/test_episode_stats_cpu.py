"""Why episodes end (include/bez_sim.h: BEZ_END_*, BezEpisodeTensor, BEZ_FLAG_REWARD_TERMS) without a GPU: the C header against abi.py,
the binding, a numpy restatement of the reward's termination tests and term split checked against the reference's golden vectors,
the env.debug.rewards mapping, and the PPO epoch row / observer tags."""
import json
import os
import re

import numpy as np
import torch

from bez_isaacgym_amd import abi
from tests.fake_env import FakeVecEnv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = open(os.path.join(ROOT, "include", "bez_sim.h")).read()
SIM_HIP = open(os.path.join(ROOT, "bez_isaacgym_amd", "csrc", "bez_sim.hip")).read()
MODEL = json.load(open(os.path.join(ROOT, "bez_isaacgym_amd", "model", "bez_model.json")))
F = np.float32


# ---------------------------------------------------------------------------------------------------- the restatement
def kick_params(max_len=900):
    c = abi.default_config(1)
    return dict(max_len=max_len, bez_init=np.array(c.bez_init[:], F), ball_init=np.array(c.ball_init[:], F), goal=np.array(c.goal[:], F))


def task_params(max_len=600, goal_angle=1.5708):
    c = abi.default_config(1)
    return dict(max_len=max_len, bez_init=np.array(c.bez_init[:], F), goal_angle=F(goal_angle))


def end_causes(task, x, prm):
    """fp32 numpy restatement of reward_of (bez_kernels.h) for N envs.  x: root (N,3), q (N,4) xyzw, v (N,3), w (N,3), dof (N,18),
    progress (N,), reset (N,) [the reset_buf the reward sees], goal (N,2) [walk / orient], ball (N,3), ball_v (N,3) [kick].
    Returns dict(bits (N,) int, terms (N,5) shaping slots 0-4, rew (N,) the deciding cause's rule / the shaping sum, margin (N,) the
    smallest relative distance of any tested quantity from its threshold)."""
    n = len(x["root"])
    d = np.asarray(MODEL["dof_default"], F)[None, :] - np.asarray(x["dof"], F)
    pn = np.sum(d * d, axis=1, dtype=F)
    root, v, w = np.asarray(x["root"], F), np.asarray(x["v"], F), np.asarray(x["w"], F)
    progress, reset = np.asarray(x["progress"], np.int64), np.asarray(x["reset"], np.int64)
    vel_reward = np.sqrt(np.sum(v * v, 1) + np.sum(w * w, 1)).astype(F)
    pos_reward = np.sqrt(pn).astype(F)
    bits = np.where(reset != 0, 1 << abi.END_CARRIED, 0).astype(np.int64)
    terms = np.zeros((n, 5), F)
    tests = []   # (quantity, threshold, fires, cause, reward)
    win = lambda scale: F(scale) - F(scale) * (progress.astype(F) / F(prm["max_len"]))
    with np.errstate(all="ignore"):
        if task == abi.TASK_KICK:
            ball, bv = np.asarray(x["ball"], F), np.asarray(x["ball_v"], F)
            dbx, dby = ball[:, 0] - root[:, 0], ball[:, 1] - root[:, 1]
            dbn = np.sqrt(dbx * dbx + dby * dby)
            vel_fwd = (dbx / dbn) * v[:, 0] + (dby / dbn) * v[:, 1]
            dgx, dgy = prm["goal"][0] - ball[:, 0], prm["goal"][1] - ball[:, 1]
            dgn = np.sqrt(dgx * dgx + dgy * dgy)
            b2gx, b2gy = dgx / dgn, dgy / dgn
            ball_fwd = b2gx * bv[:, 0] + b2gy * bv[:, 1]
            ig = prm["goal"][:2] - prm["ball_init"][:2]
            ang_init = np.arctan2(F(ig[1] / np.hypot(*ig)), F(ig[0] / np.hypot(*ig))).astype(F)
            angle_diff = np.abs(ang_init - np.arctan2(b2gy, b2gx))
            height = np.abs(F(0.325) - root[:, 2])
            kicked = np.sqrt((ball[:, 0] - prm["ball_init"][0]) ** 2 + (ball[:, 1] - prm["ball_init"][1]) ** 2)
            after = kicked > F(0.3)
            terms[:, 0] = ball_fwd * F(0.1)
            terms[:, 1] = np.where(after, F(0), vel_fwd * F(0.05))
            terms[:, 2] = -height
            terms[:, 3] = np.where(after, -(vel_reward * F(0.05)), F(0))
            terms[:, 4] = np.where(after, -(pos_reward * F(0.05)), F(0))
            drift = np.sqrt((root[:, 0] - prm["bez_init"][0]) ** 2 + (root[:, 1] - prm["bez_init"][1]) ** 2)
            tests = [(root[:, 2], 0.275, root[:, 2] < F(0.275), abi.END_FALL, F(-1)),
                     (drift, 0.5, drift > F(0.5), abi.END_OUT_OF_BOUNDS, F(-1)),
                     (angle_diff, 1.5708, angle_diff > F(1.5708), abi.END_OFF_COURSE, F(-1)),
                     (dgn, 0.05, dgn < F(0.05), abi.END_GOAL, win(100.0))]
        else:
            q, goal = np.asarray(x["q"], F), np.asarray(x["goal"], F)
            gx, gy = goal[:, 0] - root[:, 0], goal[:, 1] - root[:, 1]
            gn = np.sqrt(gx * gx + gy * gy)
            ux, uy = gx / gn, gy / gn
            qx, qy, qz, qw = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
            sy, cy = F(2) * (qw * qz + qx * qy), qw * qw + qx * qx - qy * qy - qz * qz
            hn = F(1) / np.sqrt(sy * sy + cy * cy)
            ang_goal = prm["goal_angle"] - np.arctan2(sy * hn, cy * hn)
            up_proj = F(1) - F(2) * (qx * qx + qy * qy)
            dh = np.abs(F(1) - up_proj)
            vel_lin, vel_ang = np.sqrt(np.sum(v * v, 1)), np.sqrt(np.sum(w * w, 1))
            if task == abi.TASK_WALK:
                near_q = gn
                vfwd = ux * v[:, 0] + uy * v[:, 1]
                terms[:, 1] = np.where(gn < F(0.05), F(0), vfwd * F(10))
                terms[:, 4] = np.where(gn < F(0.05), -(pos_reward * F(0.05)), -(F(5) * (pos_reward * F(0.05))))
            else:
                near_q = ang_goal
                terms[:, 0] = np.where(ang_goal < F(0.05), F(0), np.abs(ang_goal) * F(-0.5))
                terms[:, 4] = np.where(ang_goal < F(0.05), -(pos_reward * F(0.05)), -(F(0.05) * (pos_reward * F(0.05))))
            near = near_q < F(0.05)
            terms[:, 2] = -dh
            terms[:, 3] = np.where(near, -(vel_reward * F(0.05)), F(0))
            state = near & (pos_reward < F(0.15)) & (vel_ang < F(0.1)) & (vel_lin < F(0.1))
            # the goal test's margin: the four quantities it thresholds
            gm = np.min(np.stack([np.abs(near_q - F(0.05)) / F(0.05), np.abs(pos_reward - F(0.15)) / F(0.15),
                                  np.abs(vel_ang - F(0.1)) / F(0.1), np.abs(vel_lin - F(0.1)) / F(0.1)]), 0)
            tests = [(up_proj, 0.7, up_proj < F(0.7), abi.END_FALL, F(-100)), (None, gm, state, abi.END_GOAL, win(1000.0))]
            if task == abi.TASK_WALK:
                gnn = np.sqrt(goal[:, 0] ** 2 + goal[:, 1] ** 2)
                head = np.abs(np.arctan2(goal[:, 1] / gnn, goal[:, 0] / gnn) - np.arctan2(uy, ux))
                tests.append((head, 1.5708, head > F(1.5708), abi.END_OFF_COURSE, F(-100)))
            else:
                drift = np.sqrt((root[:, 0] - prm["bez_init"][0]) ** 2 + (root[:, 1] - prm["bez_init"][1]) ** 2)
                tests.append((drift, 0.3, drift > F(0.3), abi.END_OUT_OF_BOUNDS, F(-5)))
        tests.append((None, np.full(n, np.inf), progress >= prm["max_len"], abi.END_TIMEOUT, F(0)))
        rew = np.sum(terms, 1, dtype=F) if task == abi.TASK_KICK else None
        if task != abi.TASK_KICK:   # walk / orient: the shaping reward as the reference groups it
            rew = np.sum(terms, 1, dtype=F)
        margin = np.full(n, np.inf)
        for qty, thr, fires, cause, r in tests:   # in the reference's order: the last one that fires decides
            bits |= np.where(fires, 1 << cause, 0)
            rew = np.where(fires, r, rew).astype(F)
            m = thr if qty is None else np.abs(qty - F(thr)) / F(thr)
            margin = np.minimum(margin, np.nan_to_num(m, nan=np.inf))
    return dict(bits=bits, terms=terms, rew=rew, margin=margin)


def deciding(task, bits):
    return np.array([abi.end_cause(task, int(b)) for b in bits])


def golden_inputs(task, tag):
    """The golden set `tag` of `task` ("kick" / "walk" / "orient") as (inputs, params, golden rew, golden rst)."""
    if task == "kick":
        G = np.load(os.path.join(ROOT, "tests", "golden", "kick_env_golden.npz"))
        g = lambda k: G["rew_%s_%s" % (tag, k)]
        x = dict(root=g("root"), q=g("quat"), v=g("v_imu"), w=g("w_imu"), dof=g("dof_pos"), ball=g("ball"), ball_v=g("ball_v"),
                 reset=g("reset"), progress=g("progress"))
        return abi.TASK_KICK, x, kick_params(), g("rew"), g("rst")
    G = np.load(os.path.join(ROOT, "tests", "golden", "tasks_golden.npz"))
    g = lambda k: G["%s_%s_%s" % (task, tag, k)]
    x = dict(root=g("root"), q=g("q"), v=g("v"), w=g("w"), dof=g("dof"), goal=g("goal"), reset=g("reset"), progress=g("progress"))
    return (abi.TASK_WALK if task == "walk" else abi.TASK_ORIENT), x, task_params(), g("rew"), g("rst")


GOLDEN_SETS = [(t, tag) for t in ("kick", "walk", "orient") for tag in ("normal", "edge")]


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
class _CountingFakeEnv(FakeVecEnv):
    """FakeVecEnv with the simulator's episode statistics: every ended episode bumps episode_end_counts[cause, env] with a cause drawn
    from the env index and the step, and (terms on) the reward goes into slot 5 on ended steps, split over slots 0 / 2 otherwise."""

    def __init__(self, *a, terms=False, **kw):
        super().__init__(*a, **kw)
        self.episode_end_counts = torch.zeros(abi.END_CAUSES, self.n, dtype=torch.int64)
        self.reward_terms_buf = torch.zeros(abi.END_CAUSES, self.n, dtype=torch.float32)
        self.reward_terms_on = terms
        self.calls, self.ended = 0, []

    def step(self, actions):
        obs, rew, done, info = super().step(actions)
        causes = (torch.arange(self.n) + self.calls) % 3 + abi.END_FALL
        idx = done.nonzero().squeeze(-1)
        self.episode_end_counts[causes[idx], idx] += 1
        self.ended.append(done.sum().item())
        if self.reward_terms_on:
            d = done.bool()
            self.reward_terms_buf[5] += torch.where(d, rew, torch.zeros_like(rew))
            self.reward_terms_buf[0] += torch.where(d, torch.zeros_like(rew), 0.25 * rew)
            self.reward_terms_buf[2] += torch.where(d, torch.zeros_like(rew), rew - 0.25 * rew)
        self.calls += 1
        return obs, rew, done, info


def _agent(env, n, horizon):
    from bez_isaacgym_amd.ppo.a2c_continuous import A2CAgent
    from tests.test_ppo_cpu import _params
    agent = A2CAgent(_params(n, 4 * n, horizon=horizon), env, "cpu")
    agent.obs = agent.env_reset()
    return agent


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
