"""Why episodes end, restated in numpy: the reward's termination tests and term split (reward_of, bez_kernels.h) in fp32, and the
reference's golden sets as its inputs.  Shared by tests/test_episode_stats_cpu.py and tests/test_gpu_episode_stats.py."""
import json
import os

import numpy as np

from bez_isaacgym_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODEL = json.load(open(os.path.join(ROOT, "bez_isaacgym_amd", "model", "bez_model.json")))
F = np.float32


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
