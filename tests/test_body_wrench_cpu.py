"""The oracle's external wrenches (oracle.bez_oracle.Oracle.apply_body_forces) and the generators, bars and slips of
tests/body_wrench_ref.py, held against the fp64 oracle and its fp32 build alone (no GPU): the wrenched step of the oracle is what an
independent RNEA needs, calls add up and are resolved at the call, the wrench acts once, every case keeps >= 97 % of its envs and >= 4 of
every (body, mode) cell, the fp32 build passes the comparison it is the yardstick of (its errors per case are printed: the table
tests/test_gpu_body_wrench.py quotes), and the comparison rejects ten planted slips."""
import numpy as np
import pytest

from bez_isaacgym_amd import abi
from oracle.bez_oracle import Oracle
from tests import ball_contact_ref as B
from tests import body_wrench_ref as W
from tests import forward_dynamics_numpy as FD
from tests import generalized_forces_numpy as GF
from tests import rbd_numpy as R
from tests import step_terms as S

N = W.N


def _bare_cfg(asset, substeps=1):
    """flight's config with gains, joint friction and the speed limit switched off: the step is the bare articulated body plus armature"""
    cfg = S.step_cfg(N, asset, gravity=False, substeps=substeps)
    cfg.kp = cfg.kd = cfg.joint_friction = 0.0
    cfg.vel_limit = 1e9
    return cfg


@pytest.mark.parametrize("asset", list(S.ASSETS))
def test_the_oracle_wrench_is_what_an_independent_rnea_needs(asset):
    """fp64 oracle, flight, one substep, solo.  The finite-differenced accelerations of the step, put into tests/rbd_numpy.rnea_floating
    at the start state's velocities, need the applied wrench's generalised force (tests/generalized_forces_numpy.gf_ref of the call's own
    arrays) on the base and on every joint.  Bar: the getters round the new velocities to fp32, half an ulp of the largest velocity
    read; over h that is an acceleration error, and times the largest entry of M (the robot's mass) a force error -- 2.4e-7 / 2 /
    0.01667 x 2.57 = 1.8e-5 N for velocities in [2, 4), printed below from the case's own numbers.  Without the wrench the residual
    exceeds half the applied magnitude.  The ball: dv = F h / m, w1 = (w0 + h (T + x x F) / I) (1 - h damping), to two ulp32."""
    cfg = _bare_cfg(asset)
    st = W.case_states("flight", asset, N)
    calls, _ = W.loads("solo", asset, "bez_kick", st, 31, "easy", cfg, None, ("flight", asset, N, "bez_kick", False, False))
    T = W.tables(asset)
    model = GF.model_of(asset)
    o = Oracle(cfg)
    S.inject(o, st)
    for F, Tq, X, space in calls:
        o.apply_body_forces(F, Tq, X, space)
    o.step(st["actions"])
    rs0, ds0 = st["root_states"].astype(np.float64), st["dof_state"].astype(np.float64)
    rs1, ds1 = o.root_states.reshape(N, 2, 13).astype(np.float64), o.dof_state.reshape(N, 18, 2).astype(np.float64)
    h, arm = float(cfg.dt), float(cfg.armature)
    Q = sum(GF.gf_ref(model, rs0[:, 0], ds0, F, Tq, X, space) for F, Tq, X, space in calls)   # [force; moment about the root origin; joints]
    M = FD.M_batch(model, rs0[:64, 0], ds0[:64], None, arm)
    vmax = max(np.abs(rs1[:, 0, 7:13]).max(), np.abs(ds1[:, :, 1]).max())
    bar = 0.5 * float(np.spacing(np.float32(vmax))) / h * float(np.abs(M).max())
    body, mode = W.solo_cells(N, T.nbe)
    worst, weakest = 0.0, np.inf
    for e in np.flatnonzero(body < T.nb):
        w0, v0 = rs0[e, 0, 10:13], rs0[e, 0, 7:10]
        wdot, vdot = (rs1[e, 0, 10:13] - w0) / h, (rs1[e, 0, 7:10] - v0) / h
        a0 = np.concatenate([wdot, vdot - np.cross(w0, v0)])   # classical -> spatial acceleration of the torso origin
        qdd = (ds1[e, :, 1] - ds0[e, :, 1]) / h
        f0, tau = R.rnea_floating(model, rs0[e, 0, 3:7], np.concatenate([w0, v0]), a0, ds0[e, :, 0], ds0[e, :, 1], qdd, np.zeros(3))
        E0 = R.quat_to_mat(rs0[e, 0, 3:7])
        need = np.concatenate([E0 @ f0[3:], E0 @ f0[:3], tau + arm * qdd])
        worst = max(worst, float(np.abs(need - Q[e]).max()))
        mag = max(max(np.linalg.norm(c[0][e, body[e]]), 0.0 if c[1] is None else np.linalg.norm(c[1][e, body[e]])) for c in calls)
        weakest = min(weakest, float(max(np.linalg.norm(need[0:3]), np.linalg.norm(need[3:6]), np.abs(need[6:]).max())) / mag)
    print("%s: RNEA residual with the wrench %.2e (bar %.2e = ulp32(%.2f) / 2 / h x %.3f kg); without it >= %.2f of the applied magnitude"
          % (asset, worst, bar, vmax, np.abs(M).max(), weakest))
    assert worst <= bar, (asset, worst, bar)
    assert weakest > 0.5, weakest
    # the ball, closed form
    rot, pos = W.body_frames(asset, "bez_kick", st)
    mb, Ib = float(B.model()["ball"]["mass"]), float(B.model()["ball"]["inertia"])
    damp = 1.0 - h * float(cfg.ball_ang_damping)
    envs = np.flatnonzero(body == T.nb)
    assert len(envs) >= 20
    for e in envs:
        F, Tq, X, space = calls[mode[e]]
        f = F[e, T.nb].astype(np.float64)
        t = np.zeros(3) if Tq is None else Tq[e, T.nb].astype(np.float64)
        Rb = rot[e, T.nb]
        fw, tw = (Rb @ f, Rb @ t) if space == W.LOCAL else (f, t)
        arm_w = np.zeros(3) if X is None else (Rb @ X[e, T.nb] if space == W.LOCAL else X[e, T.nb] - pos[e, T.nb])
        lin = rs0[e, 1, 7:10] + h * fw / mb
        spin = (rs0[e, 1, 10:13] + h * (tw + np.cross(arm_w, fw)) / Ib) * damp
        np.testing.assert_allclose(rs1[e, 1, 7:10], lin, rtol=0, atol=2 * np.spacing(np.float32(np.abs(lin).max())), err_msg=str((asset, e)))
        np.testing.assert_allclose(rs1[e, 1, 10:13], spin, rtol=0, atol=2 * np.spacing(np.float32(np.abs(spin).max())), err_msg=str((asset, e)))
    u = Oracle(cfg)
    S.inject(u, st)
    u.step(st["actions"])
    np.testing.assert_array_equal(rs1[envs, 0], u.root_states.reshape(N, 2, 13)[envs, 0])   # the robot does not feel it


def _entries_as_one_call(o, asset, st):
    """the pending lists of every env as ONE call carrying the resolved sum: ENV space, per link the summed world force on the link's own
    body row at the link's origin, and the summed world torque plus the moments of the forces about that origin (fp64; one substep, where
    a moment and a force at a point are the same thing)"""
    T = W.tables(asset)
    links = B.asset_links(asset)
    rs, ds = st["root_states"].astype(np.float64), st["dof_state"].astype(np.float64)
    E, r = B.link_frames(asset, rs[:, 0, 0:3], rs[:, 0, 3:7], ds[:, :, 0])
    Eb = B.quat_to_mat(rs[:, 1, 3:7])
    F, Tq, X = (np.zeros((N, T.nbe, 3)) for _ in range(3))
    for e in range(N):
        for row in o.ext_entries(e):
            l = int(row[0])
            b, El = (T.nb, Eb[e]) if l == len(links) else (int(links[l]["body"]), E[e, l])
            F[e, b] += row[4:7]
            Tq[e, b] += row[7:10] + np.cross(El @ row[1:4], row[4:7])
    for l, L in enumerate(links):
        X[:, int(L["body"])] = r[:, l]
    X[:, T.nb] = rs[:, 1, 0:3]
    return F, Tq, X


def test_calls_add_up_and_are_resolved_at_the_call():
    """`stacked` in three calls gives the same fp64 outputs as the one call carrying the resolved sum, to 1e-12 relative (one substep);
    `late` -- the call made from another state than the one stepped from -- differs from flight's order by more than 10 x the response
    bar: points and LOCAL vectors are resolved at the call"""
    ref = W.reference(pattern="stacked", substeps=1)
    a, b = Oracle(ref.cfg()), Oracle(ref.cfg())
    for o in (a, b):
        S.inject(o, ref.states)
    for F, Tq, X, space in ref.calls:
        a.apply_body_forces(F, Tq, X, space)
    assert max(len(a.ext_entries(e)) for e in range(8)) > 3
    b.apply_body_forces(*_entries_as_one_call(a, "default", ref.states), space=W.ENV)
    a.step(ref.actions); b.step(ref.actions)
    oa, ob = S.outputs(a, N), S.outputs(b, N)
    for q in S.QUANTITIES:
        np.testing.assert_allclose(oa[q], ob[q], rtol=1e-12, atol=0, err_msg=q)
    assert np.abs(oa["root_vel"] - ref.unl64["root_vel"]).max() > 0.1   # (something was applied)
    late, flight = W.reference(scenario="late"), W.reference()
    for key in ("root_states", "dof_state", "actions"):
        np.testing.assert_array_equal(late.states[key], flight.states[key])
    bars = W.response_bars(flight)
    seen = {q: float(np.abs(late.out64[q] - flight.out64[q]).max()) for q in W.RESPONSE}
    print("late against flight's order: %s; response bars %s" % (seen, {q: bars[q][0] for q in W.RESPONSE}))
    for q in W.RESPONSE:
        assert seen[q] > 10 * bars[q][0], (q, seen[q], bars[q][0])


def test_side_effects():
    """None forces and torques change nothing; the wrench moves the robot and leaves the contact rows (free flight: zeros) alone; the
    launch drops it, so a second simulate() from the same state is the unloaded one bit for bit; the HARD_CONTACT / TGS_SOLVER oracles
    and a wrong shape or space raise and leave the state and the pending list unchanged"""
    ref = W.reference()
    o, u = Oracle(ref.cfg()), Oracle(ref.cfg())
    for x in (o, u):
        S.inject(x, ref.states)
    o.apply_body_forces(None, None, ref.calls[1][2], W.ENV)
    assert all(len(o.ext_entries(e)) == 0 for e in range(N))
    for F, Tq, X, space in ref.calls:
        o.apply_body_forces(F, Tq, X, space)
    assert all(len(o.ext_entries(e)) == 1 for e in range(N))
    o.pre_physics(ref.actions); u.pre_physics(ref.actions)
    o.simulate(); u.simulate()
    assert all(len(o.ext_entries(e)) == 0 for e in range(N))
    moved = np.abs(o.root_states - u.root_states).max() > 1e-3
    assert moved
    np.testing.assert_array_equal(o.contact_forces, u.contact_forces)
    S.inject(o, ref.states); S.inject(u, ref.states)
    o.simulate(); u.simulate()     # the second launch without a call is unforced
    for name in ("root_states", "dof_state", "contact_forces"):
        np.testing.assert_array_equal(getattr(o, name), getattr(u, name), err_msg=name)
    F = ref.calls[0][0]
    for flag in (abi.FLAG_HARD_CONTACT, abi.FLAG_TGS_SOLVER):
        cfg = ref.cfg(); cfg.flags |= flag
        r = Oracle(cfg)
        S.inject(r, ref.states)
        before = (r.root_states, r.dof_state)
        with pytest.raises(RuntimeError):
            r.apply_body_forces(F)
        assert all(len(r.ext_entries(e)) == 0 for e in range(N))
        np.testing.assert_array_equal(r.root_states, before[0]); np.testing.assert_array_equal(r.dof_state, before[1])
    with pytest.raises(ValueError):
        o.apply_body_forces(F[:, :-1])
    with pytest.raises(ValueError):
        o.apply_body_forces(F, space=2)
    assert all(len(o.ext_entries(e)) == 0 for e in range(N))
    o.apply_body_forces(F.reshape(-1, 3), space="local")   # both shapes, the space by name
    assert sum(len(o.ext_entries(e)) for e in range(N)) == int((F != 0).any(2).sum())


def test_kept_share_cells_and_the_hard_pushes():
    """every case keeps >= 97 % of its envs; every (body, mode) cell of every solo case keeps >= 4 envs (more than the outlier budget) and
    every body meets every mode in >= 5 envs; in every hard case >= 10 % of the kept envs show a saturation or lock bit that the
    unloaded twin does not have"""
    print()
    for name, kw in W.CASES.items():
        ref = W.reference(**kw)
        line = "%-36s kept=%d/%d" % (name, ref.kept.sum(), ref.n)
        assert ref.kept.mean() >= 0.97, (name, ref.kept.mean())
        if name in W.SOLO:
            c = W.cells(ref)
            every = np.zeros_like(c); np.add.at(every, (ref.body, ref.mode), 1)
            line += "  cells=%d smallest kept cell=%d" % (c.size, c.min())
            assert c.size == ref.tables.nbe * 4 and every.min() >= 5 and c.min() >= 4 > S.OUTLIER_BUDGET, (name, every.min(), c.min())
            assert ref.aimed.sum(1).max() == 1 and (ref.aimed[np.arange(ref.n), ref.body]).all()
        if name in W.HARD_CASES:
            share = float(W.new_bits(ref)[ref.kept].mean())
            line += "  new saturation / lock bits in %.1f %% of the kept envs" % (100 * share)
            assert share >= 0.10, (name, share)
        print(line)
    assert W.HARD_CASES and len(W.SOLO) >= 15
    d, c = W.reference(), W.reference(asset="cleats")
    assert d.tables.nbe * 4 == 88 and c.tables.nbe * 4 == 120
    sparse = W.reference(pattern="sparse", n=200)
    np.testing.assert_array_equal(np.flatnonzero(sparse.aimed.any(1)), S.NEIGHBOUR_ENVS)


def test_the_fp32_build_inside_the_bars():
    """every oracle case of the GPU file: the fp32 build against fp64 per quantity and per response quantity (printed: the GPU file's
    yardstick), and the fp32 build passes the comparison it is the yardstick of"""
    print()
    for name, kw in W.CASES.items():
        ref = W.reference(**kw)
        tab, rtab = S.error_table(ref), W.response_table(ref)
        rb = W.response_bars(ref)
        print("%-36s kept=%d/%d  %s" % (name, ref.kept.sum(), ref.n, "  ".join("%s=%.1e/%.1e" % (q, *tab[q]) for q in S.QUANTITIES)))
        print("%-36s response  %s" % ("", "  ".join("%s=%.1e/%.1e bar %.1e" % (q, *rtab[q], rb[q][0]) for q in W.RESPONSE)))
        W.compare(name, ref, ref.out32, ref.unl32, "fp32 build", p99=ref.n == N)


@pytest.mark.parametrize("slip", W.SLIPS)
def test_the_comparison_rejects_a_planted_slip(slip):
    ref, out, words = W.planted(slip)
    W.compare(slip, ref, ref.out32, ref.unl32, "unplanted")
    if slip == "predictor_blind":   # the decisions themselves change
        assert ((words & W.J.STATUS_BITS) != (ref.words64 & W.J.STATUS_BITS)).any((1, 2))[ref.kept].sum() >= 1
    with pytest.raises(AssertionError):
        W.compare(slip, ref, out, ref.unl32, "planted")
