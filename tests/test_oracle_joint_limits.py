"""The joint speed limit as a constraint inside the ABA and the leg <-> leg contact with an implicit joint-space part -- known answers
on the CPU oracle.  The same scenarios run on the HIP simulator in tests/test_gpu_joint_limits.py.

* `kick_env.py:327` gives every DOF a velocity limit of 2 pi rad/s; `kick_env.py:365-366` creates the robot with collision filter 0.
* What "the reaction reaches the parent" means, exactly: the accelerations one evaluation of the dynamics returns, put into an
  INDEPENDENT inverse dynamics (tests/rbd_numpy.py: link-local RNEA), must need no wrench on the floating base -- every force of a
  free-floating robot in zero gravity is internal.  A rate clamped after the step fails that by construction."""
import numpy as np
import pytest

from bez_isaacgym_amd import abi
from oracle.bez_oracle import Oracle
from tests import rbd_numpy as R
from tests.scenarios import capsule_penetration, _free_space_cfg, leg_press, make_backend, _pressed_state


def test_locked_joints_and_pressed_legs_need_no_base_wrench(model):
    """One evaluation of the full model in free space: >= 3 joints end the substep exactly ON the limit, the leg <-> leg contact is
    active, both hip-roll drives are saturated -- and the independent RNEA finds a base wrench of zero (1e-9 of a model whose joint
    torques here are 2.5 N m and whose contact forces are tens of newtons)."""
    rng = np.random.default_rng(7)
    cfg = _free_space_cfg(1)
    o = Oracle(cfg)
    h = float(cfg.dt) / cfg.substeps
    hits = 0
    for trial in range(12):
        q, qd, target, v0, quat, fast, sign = _pressed_state(model, rng)
        o.set_env_state_f64(0, [0.0, 0.0, 1.0], quat, v0[3:], v0[:3], q, qd)
        o.set_targets(target[None].astype(np.float32))
        a0, qdd, _, cf = o.forward_dynamics(0, 0, None)
        v_new = qd + h * qdd
        on = np.isclose(np.abs(v_new), float(cfg.vel_limit), rtol=0, atol=1e-9)
        f0, tau = R.rnea_floating(model, quat, v0, a0, q, qd, qdd, np.zeros(3))
        np.testing.assert_allclose(f0, 0.0, atol=2e-9)
        contact = np.abs(cf.reshape(-1, 3)[:21]).sum() > 1.0                      # leg rows carry the pair forces
        hits += int(on.sum() >= 3 and contact)
        # a locked joint's torque is whatever holds the limit -- not bounded by the drive's 2.5 N m (that is the constraint force)
    assert hits >= 8, hits


def test_a_clamped_rate_would_need_a_base_wrench(model):
    """The control of the test above: take the same evaluation WITHOUT the in-dynamics limit (vel_limit = inf), clamp the rates
    afterwards as the round-5 model did, and the effective accelerations need a base wrench of several newtons."""
    rng = np.random.default_rng(7)
    cfg = _free_space_cfg(1)
    cfg.vel_limit = 1e9
    o = Oracle(cfg)
    h = float(cfg.dt) / cfg.substeps
    q, qd, target, v0, quat, fast, sign = _pressed_state(model, rng)
    o.set_env_state_f64(0, [0.0, 0.0, 1.0], quat, v0[3:], v0[:3], q, qd)
    o.set_targets(target[None].astype(np.float32))
    a0, qdd, _, _ = o.forward_dynamics(0, 0, None)
    v_clamped = np.clip(qd + h * qdd, -2 * np.pi, 2 * np.pi)
    f0, _ = R.rnea_floating(model, quat, v0, a0, q, qd, (v_clamped - qd) / h, np.zeros(3))
    assert np.abs(f0).max() > 1.0, f0


@pytest.mark.parametrize("substeps", [2, 8])
def test_leg_press_stays_finite_and_keeps_its_momentum_oracle(model, substeps):
    """The scenario that broke the round-5 model (NaN at 8 substeps, 8 kg m/s of created momentum at 2, legs passing through each
    other): saturated hip drives press the legs together for 1.5 s while six joints are thrown against the speed limit.  What is left
    of a momentum drift is the first-order integrator's (it scales with h: the exact active-set reference, tune[22], shows the same
    floor), bounded here by 10 % of the 2.8 kg robot moving at 1 m/s."""
    n = 4
    cfg = _free_space_cfg(n, substeps=substeps)
    sim = make_backend("oracle", cfg)
    sim.step(np.zeros((n, 18), np.float32))
    r = leg_press(sim, n, model)
    assert r["finite"] and r["on_limit"] > 300, r
    assert r["dp"] < (1.0 if substeps == 2 else 0.1) and r["dL"] < (0.15 if substeps == 2 else 0.02), r


def test_momentum_drift_with_joints_on_the_limit_is_the_integrators(model):
    """Integrated form of the first test.  Semi-implicit Euler in generalised coordinates does not conserve the momentum of a
    tumbling, flailing robot exactly (the link Jacobians move under it: O(h) per unit time); what the DYNAMICS create would not vanish
    with h (a clamp takes h * excess acceleration out of a joint every substep: a finite total).  One control step from the pressed
    state with >= 3 joints per env on the limit at its end: the drift falls in proportion to the substep and is < 5e-3 at 128 substeps."""
    from tests.scenarios import body_momenta
    n = 6
    drift = {}
    for substeps in (8, 32, 128):
        rng = np.random.default_rng(11)
        cfg = _free_space_cfg(n, substeps=substeps)
        o = Oracle(cfg)
        o.step(np.zeros((n, 18), np.float32))
        dflt = np.asarray(model["dof_default"], float)
        acts = np.zeros((n, 18), np.float32)
        for e in range(n):
            q, qd, target, v0, quat, fast, sign = _pressed_state(model, rng)
            o.set_env_state_f64(e, [0.0, 0.0, 1.0], [0, 0, 0, 1], [0, 0, 0], [0, 0, 0], q, qd)
            acts[e] = (target - dflt).astype(np.float32)
        rs = o.root_states.reshape(n, 2, 13).copy(); rs[:, 1, 0:3] = (0.0, 3.0, 0.08); rs[:, 1, 7:] = 0
        o.set_root_states(rs.reshape(-1, 13))
        p0, L0 = body_momenta(o, n, model)
        o.pre_physics(acts); o.simulate()
        p1, L1 = body_momenta(o, n, model)
        qd1 = np.abs(o.dof_state.reshape(n, 18, 2)[:, :, 1])
        assert ((np.abs(qd1 - float(cfg.vel_limit)) < 1e-4).sum(1) >= 3).mean() >= 0.5, qd1
        drift[substeps] = (np.abs(p1 - p0).max(), np.abs(L1 - L0).max())
    assert drift[128][0] < 5e-3 and drift[128][1] < 1e-3, drift
    assert drift[128][0] < drift[8][0] / 6 and drift[32][0] < drift[8][0] / 2, drift


def test_exact_active_set_reference_holds_the_limit(model):
    """tune[22] (oracle only): with the lock set iterated to consistency no joint ever ends a substep beyond the limit; the shipped
    predictor misses some (tools/vlimit_probe.py has the rates) -- the bar here is that a miss is caught by the next substep, i.e. no
    joint is beyond the limit for two control steps in a row by more than the rate one substep of its drive could add."""
    n = 16
    for exact in (True, False):
        cfg = abi.default_config(n, seed=2)
        if exact:
            cfg.tune[22] = 8
        o = Oracle(cfg)
        rng = np.random.default_rng(2)
        o.step(np.zeros((n, 18), np.float32))
        worst = 0.0
        for t in range(40):
            o.step(rng.uniform(-1, 1, (n, 18)).astype(np.float32))
            ok = o.reset_buf == 0
            worst = max(worst, float((np.abs(o.dof_state.reshape(n, 18, 2)[:, :, 1]) * ok[:, None]).max()) / (2 * np.pi))
        if exact:
            assert worst <= 1.0 + 1e-6, worst
        else:
            assert worst < 8.0, worst


def test_self_contact_holds_the_legs_apart(model):
    """A hip rolling inward under its saturated drive (the DOF sweep's blocked direction; the other leg holds the default pose): with the
    contact at the ground contact's stiffness the leg capsules overlap by < 5 mm once the transient is over, at the yaml's 2 substeps,
    nothing rings, and the hip stops where the foot plates meet (8 mm apart in the default pose), far short of the commanded -0.7."""
    n = 2
    cfg = _free_space_cfg(n)
    o = Oracle(cfg)
    o.step(np.zeros((n, 18), np.float32))
    dflt = np.asarray(model["dof_default"], np.float32)
    rs = o.root_states.reshape(n, -1, 13).copy(); rs[:, 0, :] = 0; rs[:, 0, 2] = 1.0; rs[:, 0, 6] = 1.0
    rs[:, 1, :] = 0; rs[:, 1, 0:3] = (0.0, 3.0, 0.08); rs[:, 1, 6] = 1.0
    o.set_root_states(rs.reshape(-1, 13))
    ds = np.zeros((n, 18, 2), np.float32); ds[:, :, 0] = dflt
    o.set_dof_state(ds.reshape(-1, 2))
    act = np.zeros((n, 18), np.float32); act[:, 5] = -0.7
    pens, rolls = [], []
    for k in range(120):
        o.pre_physics(act); o.simulate()
        pens.append(capsule_penetration(o, n, model).max()); rolls.append(o.dof_state.reshape(n, 18, 2)[:, 5, 0].copy())
    assert max(pens[60:]) < 0.005, max(pens[60:])
    assert np.ptp(np.array(rolls[90:]), axis=0).max() < 0.01           # settled, not chattering
    assert -0.25 < rolls[-1][0] < -0.03, rolls[-1]                     # blocked by the other foot
