"""Scripted physics scenarios shared by the tests and by tools/getup_probe.py: the reference's three get-up tables played from lying
starts (resources/library/trajectories/trajectories/simulation_getup{front,back,side}.csv via tests/golden/trajectories.json,
`soccer_trajectories.py:56-91`) and the per-DOF limit sweep of `bez_isaacgym/test/test_kick_env.py:142-186` with the bars both back
ends are held to.  Both run through the SPLIT entry points (pre_physics + simulate) of an Oracle / SimAdapter object, so no fall
reset interferes."""
import json
import os

import numpy as np

from bez_isaacgym_amd import abi
from bez_isaacgym_amd.utils.trajectories import JOINT_ORDER, Trajectory

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLES = os.path.join(ROOT, "tests", "golden", "trajectories.json")
S = float(np.sqrt(0.5))
# (root quaternion xyzw, start height of the torso origin): the robot is dropped from just above its resting height
STARTS = {"getupfront": ((0.0, S, 0.0, S), 0.10), "getupback": ((0.0, -S, 0.0, S), 0.10), "getupside": ((S, 0.0, 0.0, S), 0.14)}
VARIANTS = {"yaml defaults": {}, "damping 2": {"kd": 2.0}, "effort 5 N*m": {"effort": 5.0},
            "effort 5 N*m, 24.5 rad/s": {"effort": 5.0, "vel_limit": 24.5}}


def up_z(q):
    """z component of the torso's z axis for xyzw quaternions (n, 4)."""
    return 1.0 - 2.0 * (q[:, 0] ** 2 + q[:, 1] ** 2)


def make_backend(backend, cfg, precision="f64"):
    if backend == "oracle":
        from oracle.bez_oracle import Oracle
        return Oracle(cfg, precision=precision)
    from tests.sim_adapter import SimAdapter
    return SimAdapter(cfg)


def lay_down(sim, n, name, rng):
    """Robot lying with every joint at 0 (+- 0.02 rad so that the envs differ), ball parked 2 m to the side."""
    quat, z = STARTS[name]
    rs = sim.root_states.reshape(n, -1, 13).copy()
    rs[:, 0, :] = 0
    rs[:, 0, 2] = z
    rs[:, 0, 3:7] = quat
    if rs.shape[1] > 1:
        rs[:, 1, :] = 0
        rs[:, 1, 0:3] = (0.0, 2.0, 0.08)
        rs[:, 1, 6] = 1.0
    sim.set_root_states(rs.reshape(-1, 13))
    ds = np.zeros((n, 18, 2), np.float32)
    ds[:, :, 0] = rng.uniform(-0.02, 0.02, (n, 18))
    ds[:, 1, 0] = 0
    sim.set_dof_state(ds.reshape(-1, 2))


def play(sim, n, name, model, settle=60, hold=120, trace_env=None):
    ready = dict(zip(JOINT_ORDER, model["dof_default"]))
    tr = Trajectory(json.load(open(TABLES))["simulation_" + name], ready)
    acts = tr.actions(model["dof_default"])
    zero_pose = -np.asarray(model["dof_default"], np.float32)
    seq = [zero_pose] * settle + list(acts) + [np.zeros(18, np.float32)] * hold
    max_z = np.zeros(n); max_up = np.full(n, -1.0)
    rows = []
    for k, a in enumerate(seq):
        sim.pre_physics(np.tile(np.asarray(a, np.float32), (n, 1)))
        sim.simulate()
        if k % 10 == 9 or k == len(seq) - 1:
            rs = sim.root_states.reshape(n, -1, 13)
            z, up = rs[:, 0, 2].astype(np.float64), up_z(rs[:, 0, 3:7].astype(np.float64))
            if k >= settle:
                max_z = np.maximum(max_z, z); max_up = np.maximum(max_up, up)
            if trace_env is not None:
                rows.append((k, float(z[trace_env]), float(up[trace_env])))
    rs = sim.root_states.reshape(n, -1, 13)
    z, up = rs[:, 0, 2].astype(np.float64), up_z(rs[:, 0, 3:7].astype(np.float64))
    ok = np.isfinite(z) & np.isfinite(up)
    return dict(steps=len(seq), final_z=float(np.median(z)), final_up=float(np.median(up)), max_z=float(np.median(max_z)),
                max_up=float(np.median(max_up)), standing=float(((z > 0.28) & (up > 0.9) & ok).mean()), finite=float(ok.mean()),
                final_z_minmax=[float(z.min()), float(z.max())], trace=rows)


def dof_sweep(sim, n, model, speed=3.0, hold=25, dofs=range(18)):
    """`test_motor_action_agent` (test_kick_env.py:142-186): one DOF after the other, the commanded position moves at `speed` rad/s
    to the lower limit, to the upper limit and back to the default pose while the others hold theirs.  The reference runs it on the
    floating robot and notes "better when fixBaseLink = True"; here the robot floats in zero gravity one metre above the plane (set
    cfg.gravity = 0 before creating `sim`), which takes the ground out of it without pinning the base.
    Returns per DOF: closest approach to the lower / upper limit and the final distance to the default pose (max over envs)."""
    lo, hi, dflt = (np.asarray(model[k], np.float64) for k in ("dof_lower", "dof_upper", "dof_default"))
    dt = float(sim.cfg.dt)
    out = []

    def place():
        rs = sim.root_states.reshape(n, -1, 13).copy()
        rs[:, 0, :] = 0; rs[:, 0, 2] = 1.0; rs[:, 0, 6] = 1.0
        if rs.shape[1] > 1:
            rs[:, 1, :] = 0; rs[:, 1, 0:3] = (0.0, 3.0, 0.08); rs[:, 1, 6] = 1.0
        sim.set_root_states(rs.reshape(-1, 13))
        ds = np.zeros((n, 18, 2), np.float32); ds[:, :, 0] = dflt
        sim.set_dof_state(ds.reshape(-1, 2))

    def run(cmd, d, goal):
        best = np.full(n, np.inf)
        steps = int(abs(goal - cmd[d]) / (speed * dt)) + 1
        for k in range(steps + hold):
            cmd[d] = goal if k >= steps else cmd[d] + np.sign(goal - cmd[d]) * min(speed * dt, abs(goal - cmd[d]))
            sim.pre_physics(np.tile((cmd - dflt).astype(np.float32), (n, 1)))
            sim.simulate()
            if k >= steps:
                q = sim.dof_state.reshape(n, 18, 2)[:, d, 0].astype(np.float64)
                best = np.minimum(best, np.abs(q - goal))
        return best
    for d in dofs:
        place()  # every DOF starts from the default pose at rest (a blocked sweep may leave the floating robot drifting)
        cmd = dflt.copy()
        miss_lo = run(cmd, d, lo[d])
        miss_hi = run(cmd, d, hi[d])
        back = run(cmd, d, dflt[d])
        q = sim.dof_state.reshape(n, 18, 2)[:, :, 0]
        out.append(dict(dof=int(d), name=JOINT_ORDER[d], miss_lower=float(miss_lo.max()), miss_upper=float(miss_hi.max()),
                        miss_default=float(back.max()), finite=bool(np.isfinite(q).all())))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# round 6: the two defects of the round-5 model (missing 2) as a scenario with numbers
def body_momenta(sim, n, model):
    """Linear momentum and angular momentum about the centre of mass of every env's robot, from the Isaac-visible rigid-body rows
    (origin velocity, spin) and the URDF masses / inertias -- independent of the step's own articulated-body quantities."""
    links = model["links"]
    mass = np.array([L["mass"] for L in links]); com = np.array([L["com"] for L in links]); body = np.array([L["body"] for L in links])
    inertia = np.array([[[L["inertia"][0], L["inertia"][3], L["inertia"][4]], [L["inertia"][3], L["inertia"][1], L["inertia"][5]],
                         [L["inertia"][4], L["inertia"][5], L["inertia"][2]]] for L in links])
    rb = sim.rigid_body_states.reshape(n, -1, 13).astype(np.float64)[:, body]
    q = rb[..., 3:7]
    x, y, z, w = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    R = np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], -1),
                  np.stack([2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)], -1),
                  np.stack([2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], -1)], -2)
    rc = np.einsum("nlij,lj->nli", R, com)
    pc = rb[..., 0:3] + rc
    vc = rb[..., 7:10] + np.cross(rb[..., 10:13], rc)
    p = (mass[None, :, None] * vc).sum(1)
    cm = (mass[None, :, None] * pc).sum(1) / mass.sum()
    Iw = np.einsum("nlij,ljk,nlmk->nlim", R, inertia, R)
    L = (np.cross(pc - cm[:, None], mass[None, :, None] * vc) + np.einsum("nlij,nlj->nli", Iw, rb[..., 10:13])).sum(1)
    return p, L


def _seg_closest(p1, q1, p2, q2):
    """closest points of two segments, batched (Ericson 5.1.9; the oracle's `segment_closest`)"""
    d1, d2, r = q1 - p1, q2 - p2, p1 - p2
    a = (d1 * d1).sum(-1); e = (d2 * d2).sum(-1); f = (d2 * r).sum(-1); c = (d1 * r).sum(-1); b = (d1 * d2).sum(-1)
    den = a * e - b * b
    s = np.clip(np.where(den > 1e-12, (b * f - c * e) / np.maximum(den, 1e-30), 0.0), 0, 1)
    t = (b * s + f) / e
    s = np.where(t < 0, np.clip(-c / a, 0, 1), np.where(t > 1, np.clip((b - c) / a, 0, 1), s))
    t = np.clip(t, 0, 1)
    return p1 + d1 * s[..., None], p2 + d2 * t[..., None]


def capsule_penetration(sim, n, model):
    """Deepest overlap (m, >= 0) over the model's left x right leg capsule pairs per env, from the rigid-body rows."""
    rb = sim.rigid_body_states.reshape(n, -1, 13).astype(np.float64)
    links, caps = model["links"], model["capsules"]
    q = rb[..., 3:7]
    x, y, z, w = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    R = np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], -1),
                  np.stack([2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)], -1),
                  np.stack([2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], -1)], -2)
    ends = []
    for c in caps:
        b = links[c["link"]]["body"]
        ends.append((rb[:, b, 0:3] + np.einsum("nij,j->ni", R[:, b], np.asarray(c["p0"])),
                     rb[:, b, 0:3] + np.einsum("nij,j->ni", R[:, b], np.asarray(c["p1"])), c["r"]))
    deepest = np.zeros(n)
    for ia, ib in model["capsule_pairs"]:
        ca, cb = _seg_closest(ends[ia][0], ends[ia][1], ends[ib][0], ends[ib][1])
        deepest = np.maximum(deepest, ends[ia][2] + ends[ib][2] - np.linalg.norm(ca - cb, axis=-1))
    return deepest


def leg_press(sim, n, model, steps=90, rng=None):
    """Free-floating robot in zero gravity (cfg.gravity = 0 before creating `sim`), the ball parked away.  Both hip-roll drives are
    commanded 0.6 rad INWARD -- past where the legs meet, so the saturated drives press the legs together for the whole run -- while hip
    pitch, knee and ankle targets of both legs jump by +-1.2 rad every 5 control steps, which puts those joints on the 2 pi rad/s speed
    limit.  Every force of the scenario is internal: linear and angular momentum must stay what they were.  Returns the largest drift
    of both over the run (absolute, SI), the deepest capsule overlap after the first contact transient, and how many joint samples sat
    on the speed limit."""
    rng = rng or np.random.default_rng(5)
    dflt = np.asarray(model["dof_default"], np.float64)
    lo, hi = np.asarray(model["dof_lower"], np.float64), np.asarray(model["dof_upper"], np.float64)
    rs = sim.root_states.reshape(n, -1, 13).copy()
    rs[:, 0, :] = 0; rs[:, 0, 2] = 1.0; rs[:, 0, 6] = 1.0
    if rs.shape[1] > 1:
        rs[:, 1, :] = 0; rs[:, 1, 0:3] = (0.0, 3.0, 0.08); rs[:, 1, 6] = 1.0
    sim.set_root_states(rs.reshape(-1, 13))
    ds = np.zeros((n, 18, 2), np.float32); ds[:, :, 0] = dflt
    sim.set_dof_state(ds.reshape(-1, 2))
    sim.pre_physics(np.zeros((n, 18), np.float32)); sim.simulate()
    p0, L0 = body_momenta(sim, n, model)
    vlim = float(sim.cfg.vel_limit)
    dp = np.zeros(n); dL = np.zeros(n); pen = np.zeros(n); on_limit = 0; over_limit = 0.0
    swing = np.zeros((n, 18))
    for k in range(steps):
        if k % 5 == 0:
            swing[:] = 0
            for d in (6, 7, 8, 14, 15, 16):
                swing[:, d] = rng.choice([-1.2, 1.2], n)
        cmd = np.tile(dflt, (n, 1)) + swing
        cmd[:, 5] = dflt[5] - 0.6; cmd[:, 13] = dflt[13] - 0.6      # both hip-roll axes count inward as negative (the sweep: 0.34 rad short of -0.785)
        cmd = np.clip(cmd, lo, hi)
        sim.pre_physics((cmd - dflt).astype(np.float32)); sim.simulate()
        p, L = body_momenta(sim, n, model)
        dp = np.maximum(dp, np.abs(p - p0).max(1)); dL = np.maximum(dL, np.abs(L - L0).max(1))
        qd = np.abs(sim.dof_state.reshape(n, 18, 2)[:, :, 1].astype(np.float64))
        on_limit += int((qd > 0.97 * vlim).sum()); over_limit = max(over_limit, float(qd.max() / vlim))
        if k >= 10:
            pen = np.maximum(pen, capsule_penetration(sim, n, model))
    q = sim.dof_state.reshape(n, 18, 2)[:, :, 0]
    return dict(dp=float(dp.max()), dL=float(dL.max()), penetration=float(pen.max()), on_limit=on_limit, over_limit=over_limit,
                finite=bool(np.isfinite(q).all()), hip_roll=[float(q[:, 5].min()), float(q[:, 13].min())])


def _free_space_cfg(n, seed=3, substeps=2):
    cfg = abi.default_config(n, seed=seed)
    cfg.gravity[:] = [0.0, 0.0, 0.0]
    cfg.substeps = substeps
    return cfg


def _pressed_state(model, rng):
    """Legs overlapping by a few millimetres (both hip rolls 0.25 rad inward: the capsules meet at 0.22 each), six leg joints just below the speed limit with
    their targets far ahead (saturated drives pushing them over it), the torso tumbling."""
    dflt = np.asarray(model["dof_default"], float)
    q = dflt + rng.uniform(-0.05, 0.05, 18)
    q[5] = dflt[5] - 0.25; q[13] = dflt[13] - 0.25
    qd = rng.uniform(-1.0, 1.0, 18)
    fast = [6, 7, 8, 14, 15, 16]
    sign = rng.choice([-1.0, 1.0], len(fast))
    qd[fast] = sign * 6.1
    target = dflt.copy()
    target[fast] = q[fast] + sign * 1.5
    target[5] = dflt[5] - 0.8; target[13] = dflt[13] - 0.8   # hip drives saturated inward
    v0 = np.concatenate([rng.uniform(-1, 1, 3), rng.uniform(-0.3, 0.3, 3)])
    quat = rng.normal(size=4); quat /= np.linalg.norm(quat)
    return q, qd, target, v0, quat, fast, sign


def _lie_on_back(b, n, count=None):
    """The first `count` envs (default: all): robot on its back (torso -x down), ball far away, joints at rest."""
    m = n if count is None else count
    rs = np.array(b.root_states, dtype=np.float32).reshape(n, b.nact, 13).copy()
    rs[:m, 0, 0:3] = [0.0, 0.0, 0.12]
    rs[:m, 0, 3:7] = [0.0, -np.sin(np.pi / 4), 0.0, np.cos(np.pi / 4)]   # xyzw: -90 deg about y -> torso +x points up
    rs[:m, 0, 7:13] = 0
    if b.nact > 1:
        rs[:m, 1, 0:3] = [5.0, 5.0, 0.0795]; rs[:m, 1, 7:13] = 0   # resting in contact (exactly z = R would sit on the contact on/off edge)
    b.set_root_states(rs.reshape(-1, 13))
    ds = np.array(b.dof_state, dtype=np.float32).reshape(n, 18, 2).copy(); ds[:m, :, 1] = 0
    b.set_dof_state(ds.reshape(-1, 2))
    b.set_reset(np.zeros(n, np.int64)); b.set_progress(np.zeros(n, np.int64))


def check_dof_sweep(rows):
    """Every actuated DOF reaches both limits and returns (zero gravity, floating base) -- except where the model says it cannot:
    the head joints never receive an action (kick_env.py:414), a hip rolling INWARD meets the other leg (collision_filter 0,
    kick_env.py:365-366: the foot plates, 8 mm apart in the default pose, touch first) 0.6 rad short of its -0.785 rad limit, and a hip
    yawing to its lower limit swings the hip box into the other leg 0.1 rad short of -1.309.  (Round 5's 3000 N/m explicit spring let
    the saturated drive push 2 cm into the other leg: its hip roll stopped 0.34 rad short, at the thighs.)"""
    for r in rows:
        assert r["finite"], r
        if r["dof"] < 2:
            assert r["miss_default"] < 1e-3 and r["miss_lower"] > 1.5, r       # did not move
        elif r["name"].endswith("leg_motor_1"):
            assert 0.5 < r["miss_lower"] < 0.72 and r["miss_upper"] < 0.05 and r["miss_default"] < 0.05, r
        elif r["name"].endswith("leg_motor_0"):
            assert 0.03 < r["miss_lower"] < 0.2 and r["miss_upper"] < 0.05 and r["miss_default"] < 0.05, r
        else:
            assert r["miss_lower"] < 0.05 and r["miss_upper"] < 0.05 and r["miss_default"] < 0.05, r


def check_fixed_base_sweep(rows, root_before, root_after):
    """The reference's form of the sweep ("better when fixBaseLink = True", test/test_kick_env.py:142-186): gravity on, the torso welded one
    metre above the plane.  The torso does not move by a bit; every actuated DOF reaches both limits under its limb's weight and returns,
    with the same exceptions as the floating sweep (head joints never commanded, a hip rolling inward or yawing to its lower limit meets the other leg)."""
    assert np.array_equal(root_before, root_after)
    for r in rows:
        assert r["finite"], r
        if r["dof"] < 2:
            assert r["miss_default"] < 1e-3 and r["miss_lower"] > 1.5, r
        elif r["name"].endswith("leg_motor_1"):
            assert 0.5 < r["miss_lower"] < 0.72 and r["miss_upper"] < 0.06 and r["miss_default"] < 0.06, r
        elif r["name"].endswith("leg_motor_0"):
            assert 0.03 < r["miss_lower"] < 0.2 and r["miss_upper"] < 0.06 and r["miss_default"] < 0.06, r
        else:
            assert r["miss_lower"] < 0.06 and r["miss_upper"] < 0.06 and r["miss_default"] < 0.06, r
