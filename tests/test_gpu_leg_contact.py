"""Leg <-> leg capsule contact of the fused step kernels, pair by pair, against the fp64 oracle and the numpy pair geometry of
tests/leg_contact_ref.py: every one of the 28 left-leg x right-leg capsule pairs inside the joint limits, both owners of the pairs in the
wave kernels at once (part 0: left hip, thigh and calf capsule, part 1: left ankle and foot-plate capsules; bez_kernel_ws8.h
ws_self_pairs<PART>, the hand-over of A_M / A_S by ws_pair_publish / ws_pair_wait, the lane-group copy in bez_ws_quad.inc, the
one-env-per-lane kernel in bez_kernels.h), on the default, cleats and box assets, with and without per-env parameters, at 1 - 4
substeps, with contact-free neighbours in the workgroup, with the contact switched off and with the DOF-force recording on.

Every case is ONE control step from generated states written into an fp64 Oracle, its fp32 build and the HIP sim.  Envs in which some
pair is within 0.1 mm of touching are left out (leg_contact_ref.kept: none in the zero-gravity scenarios by construction, 62 of 1000 in
the stance); the others are held to the project's single-step bars (tests/step_terms.BARS through case_bars) with
tests.parity_util.EnvOutliers' default budget, per quantity the p99 of |HIP - f64| to 2.5 x the p99 of the oracle's own fp32 build + 1e-6,
and per aimed pair the worst contact-force error to the cf bar.  The health word stays zero: a bounded spin wait that gave up
(BEZ_HEALTH_SPIN_TIMEOUT) is a failure, not noise.

What the oracle's fp32 build shows on these states (CPU, worst / p99 over the kept envs; tests/test_leg_contact_cpu.py prints the table):
    free, 2 substeps      pose 1.8e-7  root velocity 5.0e-5  q 3.5e-6  qd 4.2e-4 / 6.5e-5  contact forces 2.7e-3 / 7.2e-4 N  reward 2.5e-6
    both_parts, 1 - 4     pose 2.4e-7  root velocity 4.3e-5  q 2.5e-6  qd 3.4e-4 / 9.7e-5  contact forces 1.3e-3 / 4.7e-4 N  reward 2.1e-6
    stance, 2 substeps    pose 8.3e-6  root velocity 1.7e-3  q 8.3e-5  qd 1.0e-2 / 1.4e-3  contact forces 2.0e-2 / 7.5e-3 N  reward 8.4e-5
30 - 100 x below the bars in zero gravity, where the p99 ratio and the per-pair force check do the work; in the stance case_bars raises
the reward's bar (2e-5) to 3 x the fp32 build's worst outside the budget (4.4e-5 - 6.4e-5), nothing else.

BEZ_LEG_CONTACT_REPORT=<file>: every case appends its kept / outlier counts, per quantity the worst and p99 of the HIP kernel and of the
fp32 build, the raised bars, and where they are measured the momentum figures and the normal-direction tolerance
(profiles/leg_contact_errors.txt)."""
import numpy as np
import pytest

from bez_isaacgym_amd import abi
from tests import ball_contact_ref as B
from tests import leg_contact_ref as L
from tests import step_terms as S
from tests.step_terms import KERNELS, N, hip_sim as _hip, step_outputs as _step

pytestmark = pytest.mark.gpu

ASSETS = list(S.ASSETS)


def _note(text):
    S.note("BEZ_LEG_CONTACT_REPORT", text)


def _compare(case, ref, kernel, out, p99=True):
    def report(err, outliers, bars):
        aimed = np.bincount(ref.aim[ref.aim >= 0], minlength=L.NPAIR)
        words = S.report_words("%s %s %s" % (case, ref.asset, kernel), 32, ref, err, outliers, bars)
        words[0] += " aimed>=%d" % aimed.min()
        _note("  ".join(words))
        if kernel == KERNELS[0]:   # the case's own coverage, once
            if ref.scenario in ("both_parts", "stance"):   # no pair is aimed at: the envs in which each overlaps
                _note("%-32s envs in which pair 0..27 overlaps: %s" % ("%s %s" % (case, ref.asset), " ".join(map(str, (ref.gap < 0).sum(0)))))
            else:
                short = [p for p in range(L.NPAIR) if aimed[p] < 5] if ref.scenario == "solo" else []
                _note("%-32s envs aimed at pair 0..27: %s%s" % ("%s %s" % (case, ref.asset), " ".join(map(str, aimed)),
                                                              "  (pairs without 5 solo envs: %s)" % short if short else ""))
    return L.compare("%s %s" % (case, ref.asset), ref, out, kernel, report=report, p99=p99)


@pytest.mark.parametrize("dr", [False, True], ids=["plain", "dr"])
@pytest.mark.parametrize("asset", ASSETS)
@pytest.mark.parametrize("kernel", KERNELS)
def test_pair_by_pair(kernel, asset, dr, monkeypatch):
    """Free space, two substeps, env e with capsule pair e % 28 overlapping by 1 - 10 mm (every pair in 35 - 36 envs, up to three pairs at
    once).  plain: no per-env parameters; dr: per-env friction (it feeds self_pair), Kp and Kd scales on both sides."""
    ref = L.reference("free", asset, N, dr=dr)
    _compare("free-%s" % ("dr" if dr else "plain"), ref, kernel, _step(_hip(ref, kernel, monkeypatch), ref))


@pytest.mark.parametrize("asset", ["default", "cleats"])
@pytest.mark.parametrize("kernel", KERNELS)
def test_loaded_rows_are_the_numpy_pair(kernel, asset, monkeypatch):
    """One substep, the aimed pair the only one that overlaps (leg_contact_ref "solo"; the other envs stand with default leg joints): the
    robot rows that carry a force are exactly the aimed pair's two bodies -- or none, which the kernel may decide only where the oracle's
    force is within the bar of zero --, the two rows cancel to 1e-4 N + 1e-5 relative and so does the sum of all robot rows, and the row
    of capsule a's body points along the numpy normal b -> a, within 3 x the error of the fp32 evaluation of that normal.  Once more
    with BEZ_FLAG_CF_WITH_FRICTION: the rows still cancel and still match the oracle."""
    pb = L.pair_bodies(asset)
    nb = B.ball_row(asset)
    feet = [B.box_table(asset)[b]["body"] for b in (4, 9)]
    for flags, tag in ((0, "solo1"), (abi.FLAG_CF_WITH_FRICTION, "solo1-fric")):
        ref = L.reference("solo", asset, N, substeps=1, flags=flags)
        out = _step(_hip(ref, kernel, monkeypatch), ref)
        bad = _compare(tag, ref, kernel, out)
        cf = out["cf"].reshape(N, -1, 3)
        loaded = B.loaded_rows(cf, asset)
        e = np.flatnonzero(ref.aim >= 0)
        allowed = np.zeros_like(loaded)
        allowed[e[:, None], pb[ref.aim[e]]] = True
        assert not (loaded & ~allowed).any(), np.flatnonzero((loaded & ~allowed).any(1))
        assert (cf[:, nb] == 0).all()
        a_row, b_row = (cf[e, pb[ref.aim[e], s]] for s in (0, 1))
        # (the fused step ends with the feet-sensor noise filter, which zeroes in place the components of the two foot rows of the
        # assets without cleats that do not exceed 0.01 N: there a foot row may be zero where the other body's is within the gate)
        foot = (asset != "cleats") & np.isin(pb[ref.aim[e]], feet).any(1)[:, None]
        gated = foot & (np.abs(a_row + b_row) <= 0.01 + 1e-4) & ((a_row == 0) | (b_row == 0))
        balanced = np.abs(a_row + b_row) <= 1e-4 + 1e-5 * np.abs(a_row)
        assert (balanced | gated).all(), (e[~(balanced | gated).all(1)], (a_row + b_row)[~(balanced | gated).all(1)])
        total = cf[e, :nb].sum(1)
        assert ((np.abs(total) <= 1e-4 + 1e-5 * np.abs(a_row)) | gated).all()
        # a pair loaded on one side only belongs to a force within the bar of zero
        o_loaded = B.loaded_rows(ref.out64["cf"], asset).any(1)
        differ = ref.kept & ~bad & (o_loaded != loaded.any(1))
        f = np.maximum(np.abs(cf[:, :nb]).max((1, 2)), np.abs(ref.out64["cf"].reshape(N, -1, 3)[:, :nb]).max((1, 2)))
        assert (f[differ] <= S.BARS["cf"][0]).all(), (np.flatnonzero(differ), f[differ])
        assert loaded.any(1)[e].mean() >= 0.5
        if flags == 0:   # the normal force alone: its direction is the numpy normal
            tol, ok = L.normal_tolerance(ref)
            _note("%-32s normal-direction tolerance %.2e (3 x the fp32 evaluation's error)" % ("%s %s %s" % (tag, asset, kernel), tol))
            nrm = ref.normal[e, ref.aim[e]]
            mag = (a_row * nrm).sum(1)
            # (a foot row that the 0.01 N gate took a component from has lost its direction: left out)
            sel = ok[e, ref.aim[e]] & loaded.any(1)[e] & ~(foot[:, 0] & (a_row == 0).any(1))
            assert sel.sum() >= 200 and (mag[sel] > 0).all()
            dev = np.abs(a_row - mag[:, None] * nrm) / np.maximum(mag, 1e-30)[:, None]
            print("normal direction: worst deviation %.2e of %d rows, tolerance %.2e" % (dev[sel].max(), sel.sum(), tol))
            assert (dev[sel] <= tol).all(), (dev[sel].max(), tol)


@pytest.mark.parametrize("substeps", [1, 2, 3, 4])
@pytest.mark.parametrize("kernel", KERNELS)
def test_both_parts_and_substeps(kernel, substeps, monkeypatch):
    """A pair of part 0 and a pair of part 1 overlap in every env, in 63 envs both foot-plate capsules of one foot at once (two wrenches
    into one link), at one to four substeps: the sequence word of the hand-over advances once per substep."""
    ref = L.reference("both_parts", "default", N, substeps=substeps)
    _compare("both-s%d" % substeps, ref, kernel, _step(_hip(ref, kernel, monkeypatch), ref))


@pytest.mark.parametrize("asset", ASSETS)
@pytest.mark.parametrize("kernel", KERNELS)
def test_stance(kernel, asset, monkeypatch):
    """The reset state standing on the ground under gravity with both hip rolls turned inward: near-parallel capsules, several pairs at
    once, next to foot <-> ground contact -- what training meets at every reset."""
    ref = L.reference("stance", asset, N)
    _compare("stance", ref, kernel, _step(_hip(ref, kernel, monkeypatch), ref))


@pytest.mark.parametrize("kernel", KERNELS)
def test_contact_free_neighbours(kernel, monkeypatch):
    """Sim A: every env with a leg <-> leg contact.  Sim B: the same states with default leg joints everywhere except the first and last
    lanes of the 16- and 64-env workgroups and the last env.  Those envs agree between A and B bit for bit, and both meet the bars on
    all their envs.  (The p99 ratio is printed and reported here, not asserted: of 200 envs it is the third-worst env.  Two 200-env
    samples drawn from the fp32 build's OWN errors on the 1000 free envs differ by more than 2.5 x in their p99 in 4 % (root velocity),
    2 % (qd) and 6 % (reward) of 4000 draws, against 0.2 %, 0 and 1.4 % for samples of 1000.  Measured on A: root velocity 1.8e-5
    (ws8, ws8q) and 9.0e-6 (lane) against the fp32 build's 6.3e-6, worst 2.8e-5 against 2.3e-5 -- 2.8 x, where the same scenario at
    1000 envs, test_pair_by_pair, shows 1.0e-5 against 8.6e-6.)"""
    n = 200
    dense, sparse = L.reference("free", "default", n), L.reference("sparse", "default", n)
    a, b = _hip(dense, kernel, monkeypatch), _hip(sparse, kernel, monkeypatch)
    oa, ob = _step(a, dense), _step(b, sparse)
    envs = list(S.NEIGHBOUR_ENVS)
    np.testing.assert_array_equal(np.flatnonzero((sparse.gap < 0).any(1)), envs)
    for name in ("root_states", "dof_state", "contact_forces"):
        x, y = getattr(a, name).reshape(n, -1), getattr(b, name).reshape(n, -1)
        np.testing.assert_array_equal(x[envs].view(np.uint32), y[envs].view(np.uint32), err_msg=name)
    assert sparse.kept.all()
    _compare("sparse", sparse, kernel, ob, p99=False)
    _compare("dense200", dense, kernel, oa, p99=False)


@pytest.mark.parametrize("kernel", KERNELS)
def test_momentum(kernel, monkeypatch):
    """The contact is internal to the robot and the ball is parked: what the step changes of the robot's linear momentum and of its
    angular momentum about its centre of mass is the integrator's own error, which the oracle shows in both precisions (0.075 kg m/s,
    p99 0.062; 0.013 kg m^2/s, p99 0.009).  The kernel may show 3 x the fp32 build's max and p99."""
    ref = L.reference("free", "default", N)
    g = _hip(ref, kernel, monkeypatch)
    before = S.robot_momentum(g, N, "default")
    _step(g, ref)
    dp = L.momentum_change(before, S.robot_momentum(g, N, "default"))
    k = ref.kept
    for col, what in ((0, "linear kg m/s"), (1, "angular kg m^2/s")):
        h, c = dp[k, col], ref.dp32[k, col]
        text = "%-32s momentum %s: HIP max %.3e p99 %.3e | fp32 build max %.3e p99 %.3e" % (
            "free-plain default %s" % kernel, what, h.max(), np.quantile(h, 0.99), c.max(), np.quantile(c, 0.99))
        print(text); _note(text)
    for col in (0, 1):
        h, c = dp[k, col], ref.dp32[k, col]
        assert h.max() <= 3.0 * c.max() and np.quantile(h, 0.99) <= 3.0 * np.quantile(c, 0.99)


@pytest.mark.parametrize("kernel", KERNELS)
def test_no_self_collision_flag(kernel, monkeypatch):
    """BEZ_FLAG_NO_SELF_COLLISION on the free states.  Flag on: no robot row carries a force and the step meets the bars against the
    oracle with the flag.  Flag off: qd differs from flag on by more than 10 x its bar in at least half the envs (the fp64 oracle: 76 %,
    tests/test_leg_contact_cpu.py) -- the flag does not step the states as if the legs stood apart for nothing."""
    on_ref, off_ref = L.reference("free", "default", N, flags=L.NS), L.reference("free", "default", N)
    out_on = _step(_hip(on_ref, kernel, monkeypatch), on_ref)
    _compare("free-ns", on_ref, kernel, out_on)
    assert not B.loaded_rows(out_on["cf"], "default").any()
    out_off = _step(_hip(off_ref, kernel, monkeypatch), off_ref)
    d = np.abs(out_off["qd"] - out_on["qd"]).max(1)
    share = (d > 10 * S.BARS["qd"][0]).mean()
    print("on/off difference of qd: median %.2e, share beyond 10 x the bar %.2f" % (np.median(d), share))
    assert share >= L.NS_SHARE


@pytest.mark.parametrize("kernel", KERNELS)
def test_dof_force_recording_leaves_the_step_unchanged(kernel, monkeypatch):
    """BEZ_FLAG_DOF_FORCE selects the recording instantiations of the step kernels, which add lock branches inside the correction
    recursion of the leg <-> leg contact: with both parts in contact they leave root state, DOF state, contact rows, observations and
    reward bit for bit what the plain instantiations compute."""
    ref = L.reference("both_parts", "default", N)
    off, on = _hip(ref, kernel, monkeypatch), _hip(ref, kernel, monkeypatch, flags=abi.FLAG_DOF_FORCE)
    off.step(ref.actions); on.step(ref.actions)
    on.sim.refresh_actuator_tensors()
    assert np.abs(on.sim.actuator_tensor(abi.ACTUATOR_DOF_FORCE).cpu().numpy()).max() > 0   # the recording really ran
    for name in ("root_states", "dof_state", "contact_forces", "obs", "rew"):
        x, y = getattr(off, name), getattr(on, name)
        np.testing.assert_array_equal(x.view(np.uint32), y.view(np.uint32), err_msg=name)
    assert off.sim.health() == 0 and on.sim.health() == 0
