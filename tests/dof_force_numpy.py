"""numpy restatement of the actuator tensors' semantics (include/bez_sim.h "Actuator tensors") for UNLOCKED, UNSATURATED joints: from the
joint state before and after ONE substep, the position targets and the config.  Needs no knowledge of the step's predictors."""
import numpy as np


def restate(cfg, model, q0, qd0, q1, qd1, target, kp_scale=1.0, kd_scale=1.0, lower=None, upper=None):
    """(tau_pd, tau_net, qdd) per joint; arrays (..., 18).  tau_pd = the PD law at the end-of-substep state (the drive torque where the
    drive did not saturate); tau_net = tau_pd - cf qd+ + tau_limit(q+, qd+) (the net joint force of a joint that is neither saturated nor
    locked)."""
    q0, qd0, q1, qd1, target = (np.asarray(a, np.float64) for a in (q0, qd0, q1, qd1, target))
    h = float(cfg.dt) / int(cfg.substeps)
    lo = np.asarray(model["dof_lower"], float) if lower is None else np.asarray(lower, float)
    hi = np.asarray(model["dof_upper"], float) if upper is None else np.asarray(upper, float)
    qdd = (qd1 - qd0) / h
    pd = float(cfg.kp) * kp_scale * (target - q1) - float(cfg.kd) * kd_scale * qd1
    cf = float(cfg.joint_friction) / np.maximum(np.abs(qd0), float(cfg.jfric_veps))
    lim = lambda b: float(cfg.limit_k) * (b - q1) - float(cfg.limit_d) * qd1
    tl = np.where(q0 < lo, lim(lo), np.where(q0 > hi, lim(hi), 0.0))
    return pd, pd - cf * qd1 + tl, qdd


def easy_subset(cfg, pd, qd1):
    """joints that end the substep more than 1e-3 rad/s off the speed limit and whose restated PD torque is inside 0.8 x effort"""
    return (np.abs(np.abs(qd1) - float(cfg.vel_limit)) > 1e-3) & (np.abs(pd) < 0.8 * float(cfg.effort))


def rnea_torques(R, model, cfg, rs0, rs1, ds0, ds1, gravity=(0.0, 0.0, 0.0)):
    """joint torques (n, 18) and qdd of the independent inverse dynamics on the states read before / after one substep of h = dt"""
    n = ds0.shape[0]
    h = float(cfg.dt) / int(cfg.substeps)
    tau = np.zeros((n, 18)); qdd = (ds1[:, :, 1] - ds0[:, :, 1]) / h
    for e in range(n):
        quat = rs0[e, 0, 3:7]; w0, v0 = rs0[e, 0, 10:13], rs0[e, 0, 7:10]
        wdot = (rs1[e, 0, 10:13] - w0) / h; vdot = (rs1[e, 0, 7:10] - v0) / h
        a0 = np.concatenate([wdot, vdot - np.cross(w0, v0)])
        _, tau[e] = R.rnea_floating(model, quat / np.linalg.norm(quat), np.concatenate([w0, v0]), a0, ds0[e, :, 0], ds0[e, :, 1], qdd[e],
                                    np.asarray(gravity, float))
    return tau, qdd


def inject_pressed(sim, n, model, seed, pressed_state, hips_default=True):
    """n states of tests/scenarios._pressed_state through the Isaac-layout setters, the hip rolls and their targets left at the
    default pose (legs apart) when `hips_default`; returns the action rows that produce the targets"""
    rng = np.random.default_rng(seed)
    dflt = np.asarray(model["dof_default"], float)
    rs = sim.root_states.reshape(n, 2, 13).copy()
    ds = np.zeros((n, 18, 2), np.float32)
    acts = np.zeros((n, 18), np.float32)
    for e in range(n):
        q, qd, target, v0, quat, fast, sign = pressed_state(model, rng)
        if hips_default:
            q[5] = dflt[5]; q[13] = dflt[13]; target[5] = dflt[5]; target[13] = dflt[13]
        rs[e, 0, 0:3] = (0.0, 0.0, 1.0); rs[e, 0, 3:7] = quat; rs[e, 0, 7:10] = v0[3:]; rs[e, 0, 10:13] = v0[:3]
        rs[e, 1, :] = 0; rs[e, 1, 0:3] = (0.0, 3.0, 0.08); rs[e, 1, 6] = 1.0
        ds[e, :, 0] = q; ds[e, :, 1] = qd
        acts[e] = (target - dflt).astype(np.float32)
    sim.set_root_states(rs.reshape(-1, 13)); sim.set_dof_state(ds.reshape(-1, 2))
    return acts
