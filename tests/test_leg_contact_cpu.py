"""The leg-contact state generators and the numpy pair geometry of tests/leg_contact_ref.py, held against the fp64 oracle and its fp32
build alone (no GPU): the generated states reach every one of the 28 capsule pairs inside the joint limits, the numpy gaps say which
body rows the oracle loads, the fp32 build's errors per scenario are printed (the yardstick of tests/test_gpu_leg_contact.py, which
runs the same states through the step kernels), and the comparison helper rejects three planted slips."""
import numpy as np
import pytest

from bez_isaacgym_amd import abi
from tests import ball_contact_ref as B
from tests import leg_contact_ref as L
from tests import proximity_numpy as P
from tests import step_terms as S

N = L.N
# the pairs the standing reset pose reaches with the hip rolls turned inward by up to 0.17 rad, each leg by its own draw: 16 of 28;
# pairs 0 - 2, 5 - 7, 12, 13, 18, 19, 22 and 23 are out of its reach
STANCE_PAIRS = {3, 4, 8, 9, 10, 11, 14, 15, 16, 17, 20, 21, 24, 25, 26, 27}


def _gaps(st, asset="default"):
    return L.pair_geometry(st["root_states"][:, 0, 3:7], st["dof_state"][:, :, 0], asset)


def test_leg_geometry_is_the_same_table_in_every_asset():
    """capsules, pairs and the kinematics of the twelve leg links: what lets one posture pool serve the three assets"""
    ref = P.tables("default")
    leg_links = [l + 1 for l in L.LEGS]
    for asset in ("cleats", "box"):
        T = P.tables(asset)
        for k in ("cap_link", "cap_p0", "cap_p1", "cap_r", "pairs"):
            np.testing.assert_array_equal(T[k], ref[k], err_msg=k)
        for l in leg_links:
            for k in ("parent", "axis", "xyz"):
                np.testing.assert_array_equal(T["links"][l][k], ref["links"][l][k])
                np.testing.assert_array_equal(np.asarray(B.asset_links(asset)[l][k], np.float64), ref["links"][l][k])
    assert sorted(set(ref["cap_link"])) == [l for l in leg_links if l not in (5, 13)]   # the hip-yaw links carry no capsule
    assert (L.PART == 0).sum() == 13 and (L.PART == 1).sum() == 15
    names = [B.asset_links("default")[l]["name"] for l in ref["cap_link"]]
    assert tuple((names[a], names[b]) for a, b in ref["pairs"]) == abi.PROX_PAIR_BODIES


def test_hip_roll_sign_brings_the_legs_together():
    dflt = np.asarray(P.MODEL["dof_default"], np.float64)
    q = np.tile(dflt, (2, 1))
    for s in (0, 1):
        q[s, L.HIP_ROLLS[0]] += (1 - 2 * s) * L.HIP_ROLL_INWARD[0] * 0.17
        q[s, L.HIP_ROLLS[1]] += (1 - 2 * s) * L.HIP_ROLL_INWARD[1] * 0.17
    gap, _, _ = L.pair_geometry(L._identity(2), q)
    assert gap[0].min() < 0 < gap[1].min()


def test_free_reaches_every_pair_inside_the_joint_limits():
    st = L.free_states(N)
    gap, sin2, _ = _gaps(st)
    env = np.arange(N)
    counts = np.bincount(st["aim"], minlength=L.NPAIR)
    assert counts.min() >= 35, counts
    aimed = gap[env, st["aim"]]
    assert (aimed <= -L.AIM_DEPTH[0]).all() and (aimed >= -L.AIM_DEPTH[1]).all(), (aimed.min(), aimed.max())
    ov = gap < 0
    assert (ov.sum(1) <= 3).all() and gap.min() >= -L.MAX_DEPTH and (np.abs(gap) >= L.CLEAR).all()
    assert (sin2[ov] >= P.PAIR_MIN_SIN2).all()
    q = st["dof_state"][:, :, 0]
    lo, hi = np.asarray(P.MODEL["dof_lower"]), np.asarray(P.MODEL["dof_upper"])
    assert (q[:, L.LEGS] >= lo[L.LEGS]).all() and (q[:, L.LEGS] <= hi[L.LEGS]).all()
    assert L.kept(gap).all()
    # distinct postures: the pool is not one posture repeated
    for p in range(L.NPAIR):
        assert len(np.unique(q[st["aim"] == p][:, L.LEGS], axis=0)) >= 30, p
    print("envs per pair", counts.tolist(), " pairs overlapping per env: 1 / 2 / 3 =", np.bincount(ov.sum(1), minlength=4)[1:].tolist())


def test_solo_pairs():
    st = L.case_states("solo", "default", N)
    gap, _, _ = _gaps(st)
    ov = gap < 0
    solo = st["aim"] >= 0
    assert (ov.sum(1)[solo] == 1).all() and ov[solo, st["aim"][solo]].all() and not ov[~solo].any()
    assert L.kept(gap).all() and (np.abs(gap) >= L.CLEAR).all()
    counts = np.bincount(st["aim"][solo], minlength=L.NPAIR)
    without = [p for p in range(L.NPAIR) if counts[p] < 5]
    print("solo envs per pair", counts.tolist(), " pairs without 5 solo envs:", without)
    assert len(without) <= 3, without


def test_both_parts():
    st = L.both_parts_states(N)
    gap, sin2, _ = _gaps(st)
    ov = gap < 0
    assert L.parts_both(gap).sum() >= 100 and (L.plates_both(gap) & L.parts_both(gap)).sum() >= 30
    np.testing.assert_array_equal(L.plates_both(gap), st["plates"])
    assert (ov.sum(1) <= 5).all() and (ov.sum(1) >= 2).all() and gap.min() >= -L.MAX_DEPTH
    assert L.kept(gap).all() and (sin2[ov] >= P.PAIR_MIN_SIN2).all()
    print("both parts %d, both plates of a foot %d, pairs per env 2..5 = %s" % (L.parts_both(gap).sum(), st["plates"].sum(),
                                                                               np.bincount(ov.sum(1), minlength=6)[2:].tolist()))


@pytest.mark.parametrize("asset", list(S.ASSETS))
def test_stance_keeps_nine_in_ten_and_reaches_half_the_pairs(asset):
    ref = L.reference("stance", asset, N)
    assert ref.kept.mean() >= 0.90, ref.kept.mean()
    reached = set(np.flatnonzero((ref.gap < 0).any(0)).tolist())
    print("stance %s: kept %d of %d, pairs reached %s" % (asset, ref.kept.sum(), N, sorted(reached)))
    assert reached <= STANCE_PAIRS and len(reached) >= 10, sorted(reached)


def test_the_oracle_loads_the_aimed_pair():
    """one substep: the aimed pair's two body rows carry a force in at least 75 % of the free envs and in at least 5 envs of every pair
    (the others separate fast enough for the contact law to give no force)"""
    ref = L.reference("free", "default", N, substeps=1)
    loaded = np.abs(L.aimed_rows(ref.out64["cf"], ref)).max((1, 2)) > 0
    per_pair = np.bincount(ref.aim[loaded], minlength=L.NPAIR)
    print("aimed pair loaded in %.1f %% of the envs; per pair %s" % (100 * loaded.mean(), per_pair.tolist()))
    assert loaded.mean() >= 0.75 and per_pair.min() >= 5


@pytest.mark.parametrize("asset", ["default", "cleats"])
def test_numpy_gaps_say_which_rows_the_oracle_loads(asset):
    """solo, one substep: the loaded robot rows are the aimed pair's two bodies or none, equal and opposite; an env whose legs stand
    in the default posture loads none"""
    ref = L.reference("solo", asset, N, substeps=1)
    nb = B.ball_row(asset)
    cf = ref.out64["cf"].reshape(N, -1, 3)
    loaded = B.loaded_rows(cf, asset)
    pb = L.pair_bodies(asset)
    assert not loaded[ref.aim < 0].any()
    allowed = np.zeros_like(loaded)
    e = np.flatnonzero(ref.aim >= 0)
    allowed[e[:, None], pb[ref.aim[e]]] = True
    assert not (loaded & ~allowed).any()
    assert np.isin(loaded.sum(1), (0, 2)).all()
    # (the step ends with the feet-sensor noise filter, which zeroes the components of the two foot rows of the assets without cleats
    # that do not exceed 0.01 N: there the other body's component stands alone)
    total = cf[:, :nb].sum(1)
    feet = [B.box_table(asset)[b]["body"] for b in (4, 9)]
    gated = (asset != "cleats") & np.isin(pb[np.maximum(ref.aim, 0)], feet).any(1)[:, None] & (np.abs(total) <= 0.01 + 1e-4)
    assert ((np.abs(total) <= 1e-4) | gated).all()
    assert (cf[:, nb] == 0).all()
    assert loaded.any(1)[e].mean() >= 0.5


def test_no_env_resets_and_the_fp32_build_stays_inside_the_bars():
    """every oracle case of the GPU file: no env resets, and the fp32 build against fp64 per quantity (printed: the GPU file's yardstick);
    the bars as step_terms.case_bars yields them -- raised nowhere in the zero-gravity scenarios up to two substeps, where the
    fp32 build sits 30 - 100 x below them, and in the stance only for the reward"""
    print()
    for case in L.CASES:
        ref = L.reference(*case)
        name = L.case_name(*case)
        assert not ref.out64["reset"].any() and not ref.out32["reset"].any(), name
        if case[0] in ("free", "solo", "both_parts"):
            assert ref.kept.all(), name
        tab = S.error_table(ref)
        bars = S.case_bars(ref)
        raised = {q: "%.1e" % bars[q][0] for q in S.QUANTITIES if bars[q][0] != S.BARS[q][0]}
        print("%-26s kept=%d/%d  %s  raised=%s" % (name, ref.kept.sum(), ref.n, "  ".join("%s=%.1e/%.1e" % (q, *tab[q]) for q in S.QUANTITIES), raised or "none"))
        if case[0] == "stance":
            assert set(raised) <= {"rew"}, (name, raised)
        elif case[3] <= 2:
            assert not raised, (name, raised)
        # the fp32 build passes the comparison it is the yardstick of
        L.compare(name, ref, ref.out32, "fp32 build")


def test_momentum_of_the_oracle():
    """the contact is internal to the robot: what the free step changes of its momentum is the integrator's own error, the same in both
    precisions (printed: the figures the GPU test multiplies by 3)"""
    ref = L.reference("free", "default", N)
    for name, dp in (("f64", ref.dp64), ("f32", ref.dp32)):
        print("%s: linear max %.3e p99 %.3e kg m/s, angular max %.3e p99 %.3e kg m^2/s" % (
            name, dp[:, 0].max(), np.quantile(dp[:, 0], 0.99), dp[:, 1].max(), np.quantile(dp[:, 1], 0.99)))
    np.testing.assert_allclose(ref.dp32, ref.dp64, atol=1e-4)


def test_switching_the_contact_off_moves_the_joints():
    """the share of free envs whose qd differs between contact on and off by more than 10 x the bar, in the fp64 oracle at 2 substeps:
    what test_no_self_collision_flag asks of the kernels"""
    on, off = L.reference("free", "default", N), L.reference("free", "default", N, flags=L.NS)
    d = np.abs(on.out64["qd"] - off.out64["qd"]).max(1)
    share = (d > 10 * S.BARS["qd"][0]).mean()
    print("median on/off difference of qd %.2e rad/s, share beyond 10 x the bar %.2f" % (np.median(d), share))
    assert share >= L.NS_SHARE


@pytest.mark.parametrize("slip", L.SLIPS)
def test_the_comparison_rejects_a_planted_slip(slip):
    ref, out = L.planted(slip)
    L.compare(slip, ref, ref.out32, "unplanted")
    with pytest.raises(AssertionError):
        L.compare(slip, ref, out, "planted")


def test_normal_tolerance():
    """the error of the pair normal evaluated in fp32, on the solo states: the tolerance of the GPU file's direction check"""
    ref = L.reference("solo", "default", N, substeps=1)
    tol, ok = L.normal_tolerance(ref)
    e = np.flatnonzero(ref.aim >= 0)
    print("normal-direction tolerance %.2e; pair_ok in %d of %d solo envs" % (tol, ok[e, ref.aim[e]].sum(), len(e)))
    assert 0 < tol < 1e-3 and ok[e, ref.aim[e]].mean() >= 0.9
