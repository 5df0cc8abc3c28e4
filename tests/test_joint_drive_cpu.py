"""The joint-drive state generators and the decision margins of tests/joint_drive_ref.py, held against the fp64 oracle and its fp32
build alone (no GPU): every case keeps at least 95 % of its envs and at least 8 of every aimed (joint, regime), the aimed regime is the
one the fp64 oracle really takes, the margin constants reproduce, the fp32 build passes the comparison it is the yardstick of (its
errors per case are printed: the table tests/test_gpu_joint_drive.py quotes), and the comparison rejects twelve planted slips."""
import numpy as np
import pytest

from bez_isaacgym_amd import abi
from tests import joint_drive_ref as J
from tests import step_terms as S

N = J.N
AIMED = [c for c in J.CASES if c[0] in ("limits", "drive", "friction")]


def test_generated_states_are_what_the_scenarios_say():
    lo, hi = J.model_limits()
    env = np.arange(N)
    for dr in (False, True):
        ref = J.reference("limits", "default", N, dr=dr)
        q = ref.states["dof_state"][:, :, 0].astype(np.float64)
        elo = lo[None] if not dr else ref.params[abi.PARAM_DOF_LOWER].astype(np.float64)
        ehi = hi[None] if not dr else ref.params[abi.PARAM_DOF_UPPER].astype(np.float64)
        below, above = elo - q, q - ehi
        a, r = ref.aim, ref.regime
        for reg, d in ((J.BELOW, below), (J.ABOVE, above)):
            x = d[env, a][r == reg]
            assert (x >= J.BEYOND[0] - 1e-6).all() and (x <= J.BEYOND[1] + 1e-6).all(), (dr, reg, x.min(), x.max())
        others = np.ones((N, J.ND), bool); others[env[r != J.INSIDE], a[r != J.INSIDE]] = False
        assert (below[others] <= -J.BOUND_SHIFT[0]).all() and (above[others] <= -J.BOUND_SHIFT[0]).all()
        if dr:   # the posture inside the model's limits, every bound of every env off the model's
            assert (q >= lo + J.LIMIT_MARGIN - 1e-6).all() and (q <= hi - J.LIMIT_MARGIN + 1e-6).all()
            assert (elo != lo[None]).all() and (ehi != hi[None]).all()
        rate = ref.states["dof_state"][env, a, 1][r != J.INSIDE]
        assert (rate > 0.5).any() and (rate < -0.5).any()    # toward and away from the bound
    cfg = J.reference("friction", "default", N).cfg()
    st = J.reference("friction", "default", N).states
    speed = np.abs(st["dof_state"][env, st["aim"], 1])
    assert speed.min() < 0.15 * cfg.jfric_veps and speed.max() > 7 * cfg.jfric_veps
    tgt = J.targets_of(st["actions"])
    assert np.abs(tgt[env, st["aim"]] - st["dof_state"][env, st["aim"], 0]).max() <= 2.4e-7    # the target on q (one fp32 rounding of a + default)
    st = J.reference("drive", "default", N).states
    lock = st["regime"] >= J.LOCK_POS
    share = np.abs(st["dof_state"][env, st["aim"], 1])[lock] / cfg.vel_limit
    assert (share >= J.LOCK_RATE[0] - 1e-6).all() and (share <= J.LOCK_RATE[1] + 1e-6).all()
    for name in ("limits", "drive", "friction"):   # the legs apart, the ball away
        st = J.reference(name, "default", N).states
        gap, _, _ = J.pair_geometry(st["root_states"][:, 0, 3:7], st["dof_state"][:, :, 0], "default")
        assert gap.min() >= J.LEG_CLEAR
        assert np.allclose(np.linalg.norm(st["root_states"][:, 1, 0:3] - st["root_states"][:, 0, 0:3], axis=1), J.BALL_AWAY)


def test_kept_share_coverage_and_the_regimes_really_taken():
    """each case keeps >= 95 % of its envs; every aimed (joint, regime) keeps >= 8 envs; the fp64 decision word of the aimed joint shows
    its regime in >= 90 % of its kept envs (friction: |qd| on the aimed side of jfric_veps); a contact row
    (legs that meet within the step) in at most 5 % of the envs of the zero-gravity cases; pressed: some joint locked and some joint saturated in >= 90 % of the kept envs"""
    print()
    for case in J.CASES:
        ref = J.reference(*case)
        name = J.case_name(*case)
        counts = J.regime_counts(ref)
        print("%-34s kept=%d/%d  %s" % (name, ref.kept.sum(), ref.n, "  ".join("%s=%d(%d)" % (k, a, b) for k, (a, b) in counts.items())))
        assert ref.kept.mean() >= 0.95, (name, ref.kept.mean())
        if case in AIMED:
            for j in range(J.ND):
                for r, reg in enumerate(J.REGIMES[case[0]]):
                    got = int((ref.kept & (ref.aim == j) & (ref.regime == r)).sum())
                    assert got >= 8, (name, j, reg, got)
            touched = np.abs(ref.out64["cf"]).max(1) > 0    # (legs that start CLEAR apart and meet within the step)
            assert touched.mean() <= 0.05, (name, touched.sum())
        if case in AIMED or case[0] == "pressed":
            for reg, (aimed, shown) in counts.items():
                assert shown >= 0.9 * aimed, (name, reg, aimed, shown)
    ref = J.reference("friction", "default", N)
    e = np.arange(N)
    side = ref.states["dof_state"][e, ref.aim, 1].__abs__() > ref.cfg().jfric_veps
    np.testing.assert_array_equal(side.astype(int), ref.regime)


def test_the_margin_constants_reproduce():
    """measure_margins over every case gives what the module records (*_MEASURED: not less, and not less than half of it, so that the
    constants are the measurement and not a guess), and with the module's margins the fp32 build takes the fp64 build's decision word
    in every kept env, substep and joint of every case"""
    refs = [J.reference(*c) for c in J.CASES]
    need = J.measure_margins(refs)
    rec = {"torque": J.TORQUE_MEASURED, "rate": J.RATE_MEASURED, "angle": J.ANGLE_MEASURED, "floor": J.FLOOR_MEASURED}
    print("measured %s\nrecorded %s\nmargins  %s" % (need, rec, J.margins()))
    for k in J.KINDS:
        assert 0.5 * rec[k] <= need[k] <= rec[k], (k, need[k], rec[k])
        assert J.margins()[k] == 2 * rec[k]
    for c, ref in zip(J.CASES, refs):
        np.testing.assert_array_equal(ref.words32[ref.kept], ref.words64[ref.kept], err_msg=J.case_name(*c))


def test_the_oracle_actuator_record_is_the_restated_one():
    """the oracle's drive torque and net joint force (the test aid the GPU file compares DRIVE_TORQUE and DOF_FORCE with) against
    tests/dof_force_numpy.restate on its own states before and after one substep: unsaturated joints' drive, unlocked joints' friction
    and limit terms, to 1e-4 N m (the restatement reads the fp32 state the getters round to); saturated joints report +-effort exactly"""
    from oracle.bez_oracle import Oracle
    from tests import ball_contact_ref as B
    from tests import dof_force_numpy as D
    for scenario, dr in (("limits", True), ("drive", False)):
        ref = J.reference(scenario, "default", N, substeps=1, dr=dr)
        o = Oracle(ref.cfg())
        S.inject(o, ref.states, ref.params)
        ds0 = ref.states["dof_state"].astype(np.float64)
        o.step(ref.actions)
        ds1 = o.dof_state.reshape(N, 18, 2).astype(np.float64)
        drive, net = ref.act64
        word = ref.words64[:, 0]
        p = ref.params or {}
        pd, rnet, _ = D.restate(ref.cfg(), B.model(), ds0[:, :, 0], ds0[:, :, 1], ref.out64["q"], ref.out64["qd"], J.targets_of(ref.actions),
                                kp_scale=p.get(abi.PARAM_KP_SCALE, 1.0), kd_scale=p.get(abi.PARAM_KD_SCALE, 1.0),
                                lower=p.get(abi.PARAM_DOF_LOWER), upper=p.get(abi.PARAM_DOF_UPPER))
        del ds1
        sat, lock = (word & abi.ACTUATOR_SATURATED) != 0, (word & abi.ACTUATOR_LOCKED) != 0
        # (the oracle's getters round the state to fp32: 2.4e-7 rad x kp x scale, 7.5e-7 rad/s x kd x scale)
        assert np.abs(drive - pd)[~sat].max() < 1e-4, np.abs(drive - pd)[~sat].max()
        assert np.abs((net - drive) - (rnet - pd))[~lock].max() < 1e-4
        eff = float(ref.cfg().effort)
        assert (drive[(word & abi.ACTUATOR_SATURATED_POS) != 0] == eff).all() and (drive[(word & abi.ACTUATOR_SATURATED_NEG) != 0] == -eff).all()


def test_the_fp32_build_inside_the_bars():
    """every oracle case of the GPU file: the fp32 build against fp64 per quantity (printed: the GPU file's yardstick), no bar raised
    by step_terms.case_bars, and the fp32 build passes the comparison it is the yardstick of"""
    print()
    for case in J.CASES:
        ref = J.reference(*case)
        name = J.case_name(*case)
        tab = S.error_table(ref)
        bars = S.case_bars(ref)
        raised = {q: "%.1e" % bars[q][0] for q in S.QUANTITIES if bars[q][0] != S.BARS[q][0]}
        print("%-34s kept=%d/%d  %s  raised=%s" % (name, ref.kept.sum(), ref.n, "  ".join("%s=%.1e/%.1e" % (q, *tab[q]) for q in S.QUANTITIES),
                                                   raised or "none"))
        assert not raised, (name, raised)
        J.compare(name, ref, ref.out32, "fp32 build", p99=True)


@pytest.mark.parametrize("slip", J.SLIPS)
def test_the_comparison_rejects_a_planted_slip(slip):
    ref, out = J.planted(slip)
    J.compare(slip, ref, ref.out32, "unplanted")
    with pytest.raises(AssertionError):
        J.compare(slip, ref, out, "planted")
