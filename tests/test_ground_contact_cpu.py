"""The ground-contact state generators and the numpy contact terms of tests/ground_contact_ref.py, held against the fp64 oracle and its
fp32 build alone (no GPU): the generated states put every one of the 22 ground points under the plane alone and the robot on its
front, back and sides, the numpy active set says which body rows the oracle loads, the three friction regimes occur, no case leaves
out more than a tenth of its envs, the fp32 build's errors per case are printed (the yardstick of tests/test_gpu_ground_contact.py,
which runs the same states through the step kernels), and the comparison helper rejects ten planted slips."""
import numpy as np
import pytest

from tests import ball_contact_ref as B
from tests import ground_contact_ref as G
from tests import proximity_numpy as P
from tests import step_terms as S

N = G.N
ASSETS = list(S.ASSETS)
# the oracle's rigid-body rows are fp32: two ulps of a position below 1 m (1.2e-7) and one ulp of each quaternion component (6e-8) on a
# lever of at most 0.2 m, four components, twice (1e-7), rounded up
ROW_BAR = 5e-7


def _oracle_rows(st, asset, n):
    from oracle.bez_oracle import Oracle
    o = Oracle(S.step_cfg(n, asset, gravity=False))
    S.inject(o, st)
    return o.rigid_body_states.reshape(n, -1, 13).astype(np.float64)


@pytest.mark.parametrize("scenario", ["free", "lying"])
@pytest.mark.parametrize("asset", ASSETS)
def test_point_heights(asset, scenario):
    """the heights of the generators' own forward kinematics: the proximity reference's ground rows to its fp64 bar (1e-9), and the
    oracle's fp32 rigid-body rows applied to the points' offsets to ROW_BAR"""
    st = G.case_states(scenario, asset, N)
    h = G.heights(st, asset)
    ground = P.proximity_ref(asset, st["root_states"][:, 0], st["dof_state"], st["root_states"][:, 1, 0:3])["ground"]
    assert np.abs(h - ground[:, :, 2]).max() < 1e-9
    rb = _oracle_rows(st, asset, N)
    T = P.tables(asset)
    m = P.MODEL["cleats"] if asset == "cleats" else P.MODEL
    for i in range(G.NPT):
        # the link's row and the point's own (for the cleats asset the cleat's): both carry the link's rotation
        for b in (m["links"][T["pt_link"][i]]["body"], G.point_bodies(asset)[i]):
            x = rb[:, b, 0:3] + np.einsum("nij,j->ni", B.quat_to_mat(rb[:, b, 3:7]), T["pt_pos"][i] - np.asarray(m["body_offset"][b]))
            assert np.abs(h[:, i] - x[:, 2]).max() < ROW_BAR, (i, b, np.abs(h[:, i] - x[:, 2]).max())
    assert np.abs(h[:, G.BALL] - (rb[:, B.ball_row(asset), 2] - B.ball_radius())).max() < ROW_BAR


@pytest.mark.parametrize("asset", ASSETS)
def test_free_puts_every_point_under_the_plane_alone(asset):
    st = G.free_states(N, asset)
    h = G.heights(st, asset)
    env = np.arange(N)
    counts = np.bincount(st["aim"], minlength=G.NPT)
    assert counts.min() >= 45 and counts.max() <= 46, counts
    aimed = -h[env, st["aim"]]
    assert (aimed >= G.AIM_DEPTH[0] - 1e-6).all() and (aimed <= G.AIM_DEPTH[1] + 1e-6).all(), (aimed.min(), aimed.max())
    others = h[:, :G.NPT].copy(); others[env, st["aim"]] = np.inf
    assert others.min() >= G.CLEAR - 1e-6, others.min()
    gap, _, _ = G.pair_geometry(st["root_states"][:, 0, 3:7], st["dof_state"][:, :, 0], asset)
    assert gap.min() >= G.CLEAR
    q = st["dof_state"][:, :, 0]
    lo, hi = np.asarray(P.MODEL["dof_lower"]), np.asarray(P.MODEL["dof_upper"])
    assert (q >= lo + G.LIMIT_MARGIN - 1e-6).all() and (q <= hi - G.LIMIT_MARGIN + 1e-6).all()
    for p in range(G.NPT):   # distinct postures: the pool is not one posture repeated
        assert len(np.unique(q[st["aim"] == p], axis=0)) == counts[p], p
    ball = -h[:, G.BALL]
    assert (ball >= G.BALL_DEPTH[0] - 1e-6).all() and (ball <= G.BALL_DEPTH[1] + 1e-6).all()
    assert np.allclose(np.linalg.norm(st["root_states"][:, 1, 0:2] - st["root_states"][:, 0, 0:2], axis=1), G.BALL_AWAY)
    assert st["slow"].sum() == sum(1 for e in range(N) if (e // G.NPT) % 4 == 3) and 0.2 <= st["slow"].mean() <= 0.3
    fast, slow = (np.abs(st["dof_state"][s][:, :, 1]).max() for s in (~st["slow"], st["slow"]))
    assert slow <= G.SLOW and fast > 0.9
    print("%s: envs per point %s, depth %.2f - %.2f mm" % (asset, counts.tolist(), 1e3 * aimed.min(), 1e3 * aimed.max()))


@pytest.mark.parametrize("asset", ASSETS)
def test_lying_loads_several_bodies(asset):
    st = G.lying_states(N, asset)
    h = G.heights(st, asset)[:, :G.NPT]
    under = h < 0
    link = P.tables(asset)["pt_link"]
    nbody = sum(under[:, link == l].any(1).astype(int) for l in np.unique(link))
    assert (under.sum(1) >= 2).all() and (nbody >= 2).all() and (np.abs(h) >= G.KEPT_MARGIN).all()
    low = -h.min(1)
    assert (low >= G.LYING_DEPTH[0] - 1e-6).all() and (low <= G.LYING_DEPTH[1] + 1e-6).all()
    gap, _, _ = G.pair_geometry(st["root_states"][:, 0, 3:7], st["dof_state"][:, :, 0], asset)
    assert gap.min() >= G.CLEAR
    ub = G.under_bodies(under, asset)
    combos = {"%s+%s" % (G.BODIES[a], G.BODIES[b]): int((ub[:, a] & ub[:, b] & (ub.sum(1) == 2)).sum()) for a, b in G.LYING_COMBOS}
    print("%s: %s, three or more of torso / head / forearm / foot %d, envs per point %s, sides %s" % (
        asset, combos, (ub.sum(1) >= 3).sum(), under.sum(0).tolist(), np.bincount(st["side"], minlength=4).tolist()))
    assert min(combos.values()) >= 100, combos
    assert under.sum(0).min() >= 15, under.sum(0)
    assert np.bincount(st["side"], minlength=4).min() >= 50
    # the attitude is a side within 0.25 rad: the axis that points down stays within 0.25 rad of the vertical
    E = B.quat_to_mat(st["root_states"][:, 0, 3:7])
    down = np.where(st["side"] == 0, E[:, 2, 0], np.where(st["side"] == 1, -E[:, 2, 0], np.where(st["side"] == 2, E[:, 2, 1], -E[:, 2, 1])))
    assert (down <= -np.cos(0.25) + 1e-6).all()


def test_torso_ball_puts_the_ball_on_the_lying_torso():
    ref = G.reference("torso_ball", "default", 200)
    assert (ref.states["side"] < 2).all()
    torso = ref.depths[:, -1]
    assert (torso >= 0.4e-3).all() and (torso <= 10e-3 + 1e-6).all() and (ref.depths[:, :-1] <= -G.CLEAR + 1e-6).all()
    assert (ref.terms["d"][:, 8:16] > 0).any(1).all()                       # a torso point under the plane in every env
    assert (ref.states["root_states"][:, 1, 2] > ref.states["root_states"][:, 0, 2]).all()   # from above
    cf = ref.out64["cf"].reshape(ref.n, -1, 3)
    assert (np.abs(cf[:, 0]).max(1) > 0).mean() >= 0.5 and (np.abs(cf[:, B.ball_row("default")]).max(1) > 0).mean() >= 0.5


def test_sparse_contact_set_is_the_neighbour_envs():
    n = 200
    dense, sparse = G.reference("free", "default", n), G.reference("sparse", "default", n)
    envs = list(S.NEIGHBOUR_ENVS)
    np.testing.assert_array_equal(np.flatnonzero((sparse.terms["d"] > 0).any(1)), envs)
    np.testing.assert_array_equal(np.flatnonzero(sparse.aim >= 0), envs)
    assert (sparse.terms["height"].min(1)[sparse.aim < 0] >= G.LIFT - G.AIM_DEPTH[1] - 1e-6).all()
    for k in ("root_states", "dof_state"):
        np.testing.assert_array_equal(sparse.states[k][envs], dense.states[k][envs])
    cf = sparse.out64["cf"].reshape(n, -1, 3)
    assert not np.abs(cf[sparse.aim < 0]).any() and np.abs(cf[envs]).max((1, 2)).all()


@pytest.mark.parametrize("flags", [0, G.FRIC], ids=["normal", "fric"])
@pytest.mark.parametrize("asset", ASSETS)
def test_numpy_active_set_is_the_rows_the_oracle_loads(asset, flags):
    """solo, one substep, on the kept envs: the oracle's loaded rows (robot and ball) are the bodies of the numpy active set -- for the
    cleats asset the cleat's row and never the foot plate's; without the friction flag a loaded row has only a z component.  (The step
    ends with the feet-sensor noise filter, which zeroes the components of the two foot rows of the assets without cleats that do not
    exceed 0.01 N: there an active point may leave its row empty.)"""
    ref = G.reference("solo", asset, N, substeps=1, flags=flags)
    k = ref.kept
    nb = B.ball_row(asset)
    cf = ref.out64["cf"].reshape(N, -1, 3)
    loaded = np.abs(cf).max(2) > 0
    want = G.active_bodies(ref.terms, asset)
    feet = G.foot_plate_rows(asset)
    differ = (loaded != want)[k]
    if asset == "cleats":
        assert not loaded[:, feet].any()
    else:
        gated = np.zeros_like(want); gated[:, feet] = want[:, feet] & ~loaded[:, feet]
        print("%s: %d foot rows emptied by the 0.01 N filter" % (asset, gated[k].sum()))
        assert gated[k].sum() <= 0.02 * want[k][:, feet].sum()
        differ &= ~gated[k]
    assert not differ.any(), np.argwhere(differ)
    # the aimed point alone: at most its own row and the ball's
    assert (loaded[:, :nb].sum(1) <= 1).all()
    e = np.flatnonzero(loaded[:, :nb].any(1))
    np.testing.assert_array_equal(loaded[e, :nb].argmax(1), G.point_bodies(asset)[ref.aim[e]])
    assert loaded[:, nb].all() and len(e) >= 0.85 * N
    # pinned, not changed: the rows are not clamped at zero -- the implicit force turns negative where the step
    # accelerates the point away faster than the spring unloads; the kernels are compared on those rows like on any other
    pulling = (cf[:, :nb, 2] < 0).any(1)
    print("%s: %d envs with a row of f_z < 0, down to %.1f N" % (asset, pulling.sum(), cf[:, :nb, 2].min()))
    assert pulling.any()
    if not flags:
        assert not cf[:, :, 0:2].any()
    else:
        assert (np.abs(cf[e, :nb, 0:2]).max((1, 2)) > 0).mean() >= 0.95


def test_every_friction_regime_occurs():
    """each of the three regimes of ct = min(mu fn0 / max(vt, veps), ct_max) in at least 30 kept envs of some case; the one inside veps
    under the cap needs fn0 < ct_max veps / mu, 10 N with the default parameters -- below the 0.5 mm minimum depth -- and is reached by
    the params case"""
    dflt, params = G.reference("free", "default", N), G.reference("free", "default", N, contact=G.PARAMS)
    a, b = G.regime_counts(dflt.terms, dflt.kept), G.regime_counts(params.terms, params.kept)
    print("default parameters %s; params case %s %s" % (a, dict(G.PARAMS), b))
    assert a["slipping"] >= 30 and a["capped"] >= 30
    assert min(b.values()) >= 30, b
    # the params case changes every parameter the contact law reads
    c = G.contact_values(params.cfg())
    for k, v in G.contact_values(dflt.cfg()).items():
        assert (c[k] != v) == (k not in ("h", "mu")), k


def test_kept_cap_and_the_fp32_build_inside_the_bars():
    """every oracle case of the GPU file: at most a tenth of the envs left out, the fp32 build against fp64 per quantity (printed: the
    GPU file's yardstick), the bars as step_terms.case_bars yields them, and the fp32 build passes the comparison it is the
    yardstick of"""
    print()
    for case in G.CASES:
        ref = G.reference(*case)
        name = G.case_name(*case)
        assert ref.kept.mean() >= 0.90, (name, ref.kept.mean())
        tab = S.error_table(ref)
        bars = S.case_bars(ref)
        raised = {q: "%.1e" % bars[q][0] for q in S.QUANTITIES if bars[q][0] != S.BARS[q][0]}
        print("%-30s kept=%d/%d  %s  raised=%s" % (name, ref.kept.sum(), ref.n, "  ".join("%s=%.1e/%.1e" % (q, *tab[q]) for q in S.QUANTITIES), raised or "none"))
        print("    " + G.coverage_line(name, ref))
        if case[0] in ("free", "solo", "sparse"):
            assert not raised, (name, raised)
        G.compare(name, ref, ref.out32, "fp32 build", p99=True)


def test_momentum_residual_of_the_oracle():
    """solo with the friction in the rows, zero gravity: the change of the robot's momentum less dt x its contact rows (their moment
    about the centre of mass) is the integrator's own error, the same in both precisions (printed: the figures the GPU test multiplies
    by 3) and small against the impulse itself"""
    ref = G.reference("solo", "default", N, substeps=1, flags=G.FRIC)
    k = ref.kept
    for name, r in (("f64", ref.res64), ("f32", ref.res32)):
        print("%s: linear max %.3e p99 %.3e kg m/s, angular max %.3e p99 %.3e kg m^2/s" % (
            name, r[k, 0].max(), np.quantile(r[k, 0], 0.99), r[k, 1].max(), np.quantile(r[k, 1], 0.99)))
    np.testing.assert_allclose(ref.res32, ref.res64, atol=1e-4)
    # the rows explain the change: taking them off leaves less than the change itself wherever the impulse is beyond the residual's level
    impulse = float(ref.cfg().dt) * np.abs(ref.out64["cf"].reshape(N, -1, 3)[:, :B.ball_row("default")].sum(1)).max(1)
    zero = np.zeros_like(ref.out64["cf"])
    from oracle.bez_oracle import Oracle
    o = Oracle(ref.cfg()); S.inject(o, ref.states)
    before = S.robot_momentum(o, N, "default"); o.step(ref.actions)
    bare = G.momentum_residual(before, S.robot_momentum(o, N, "default"), ref.com, ref.point, zero, "default", float(ref.cfg().dt))
    big = k & (impulse > 2 * ref.res64[k, 0].max())
    print("impulse median %.3e kg m/s; %d envs beyond twice the residual's max" % (np.median(impulse), big.sum()))
    assert big.sum() >= 300 and (ref.res64[big, 0] < bare[big, 0]).all()


@pytest.mark.parametrize("slip", G.SLIPS)
def test_the_comparison_rejects_a_planted_slip(slip):
    ref, out = G.planted(slip)
    G.compare(slip, ref, ref.out32, "unplanted")
    with pytest.raises(AssertionError):
        G.compare(slip, ref, out, "planted")
