"""Ground contact of the fused step kernels, point by point, against the fp64 oracle and the numpy contact terms of
tests/ground_contact_ref.py: every one of the 22 ground points alone under the plane -- the feet in the leg roles, the head and the
forearms in the two-link chain roles, the torso in the root role's idle window (bez_kernel_ws8.h), summed per body into one
BodyContact {B, C, F0} by the wave kernels (bez_ws_common.inc ws_ground_points / body_contact_of / body_contact_force) where the lane
kernel keeps one Hit per point (bez_kernels.h) --, the robot lying on its front, back and sides with several bodies loaded at once,
the torso row that takes ground and ball force in one store, the cleats records, the three friction regimes, non-default contact
parameters, 1 - 4 substeps with the mean and the last substep's rows, on the default, cleats and box assets, with and without per-env
parameters, with contact-free neighbours in the workgroup, and with the DOF-force recording and the lean step on.

Every case is ONE control step from generated states written into an fp64 Oracle, its fp32 build and the HIP sim.  Envs in which some
point is within 0.1 mm of the plane, or its start-of-step normal force within 0.1 mm x kn of zero, are left out
(ground_contact_ref.kept: at most 34 of 1000, tests/test_ground_contact_cpu.py); the others are held to the project's single-step bars
(tests/step_terms.BARS through case_bars) with tests.parity_util.EnvOutliers' default budget, per quantity the p99
of |HIP - f64| to 2.5 x the p99 of the oracle's own fp32 build + 1e-6, and per aimed point the worst contact-force error to the cf
bar.  The health word stays zero.

What the oracle's fp32 build shows on these states (CPU, worst / p99 over the kept envs; tests/test_ground_contact_cpu.py prints the table):
    free, 2 substeps      pose 1.3e-6  root velocity 3.0e-4 / 4.3e-5  q 1.7e-5  qd 2.0e-3 / 2.4e-4  contact forces 1.1e-3 / 4.6e-4 N  reward 1.9e-6
    lying, 2 substeps     pose 1.1e-6  root velocity 3.0e-4 / 9.8e-5  q 2.3e-5  qd 2.8e-3 / 3.9e-4  contact forces 1.8e-3 / 4.1e-4 N
    params, 2 substeps    pose 7.7e-7  root velocity 2.0e-4 / 6.3e-5  q 2.4e-5  qd 2.9e-3 / 4.0e-4  contact forces 4.2e-3 / 2.9e-4 N  reward 2.9e-6
7 - 70 x below the bars, so the p99 ratio and the per-point force check do the work; case_bars raises no bar in any case (at four
substeps one lying env of the fp32 build flips a branch: that is what the budget is for).

BEZ_GROUND_CONTACT_REPORT=<file>: every case appends its kept / outlier counts, per quantity the worst and p99 of the HIP kernel and of
the fp32 build, the raised bars, once per case the envs per aimed point, the envs in which each point is active and the regime counts,
and where they are measured the momentum residuals (profiles/ground_contact_errors.txt)."""
import numpy as np
import pytest

from bez_isaacgym_amd import abi
from tests import ball_contact_ref as B
from tests import ground_contact_ref as G
from tests import step_terms as S
from tests.step_terms import KERNELS, N, hip_sim as _hip, step_outputs as _step

pytestmark = pytest.mark.gpu

ASSETS = list(S.ASSETS)


def _note(text):
    S.note("BEZ_GROUND_CONTACT_REPORT", text)


def _compare(case, ref, kernel, out, p99=True):
    def report(err, outliers, bars):
        _note("  ".join(S.report_words("%s %s %s" % (case, ref.asset, kernel), 36, ref, err, outliers, bars)))
        if kernel == KERNELS[0]:   # the case's own coverage, once
            _note(G.coverage_line("%s %s" % (case, ref.asset), ref))
    return G.compare("%s %s" % (case, ref.asset), ref, out, kernel, report=report, p99=p99)


@pytest.mark.parametrize("dr", [False, True], ids=["plain", "dr"])
@pytest.mark.parametrize("asset", ASSETS)
@pytest.mark.parametrize("kernel", KERNELS)
def test_point_by_point(kernel, asset, dr, monkeypatch):
    """Zero gravity, two substeps, env e with ground point e % 22 alone under the plane by 0.5 - 10 mm (every point in 45 - 46 envs), the
    ball on the ground 3 m away in every env.  plain: no per-env parameters; dr: per-env friction (it feeds the ground contact), Kp and
    Kd scales on both sides."""
    ref = G.reference("free", asset, N, dr=dr)
    _compare("free-%s" % ("dr" if dr else "plain"), ref, kernel, _step(_hip(ref, kernel, monkeypatch), ref))


@pytest.mark.parametrize("asset", ["default", "cleats"])
@pytest.mark.parametrize("kernel", KERNELS)
def test_loaded_rows_are_the_numpy_active_set(kernel, asset, monkeypatch):
    """One substep, the aimed point the only one under the plane: the robot rows that carry a force are exactly the aimed point's body
    row where the numpy active set holds it -- or none, which the kernel may decide differently from the oracle only where the oracle's
    force is within the bar of zero --, for the cleats asset the cleat's own row with the foot plate's row zero, and the ball's row is
    loaded in every kept env.  Without BEZ_FLAG_CF_WITH_FRICTION the x and y components of every row are exactly 0; with it the rows
    still match the oracle."""
    nb = B.ball_row(asset)
    pb = G.point_bodies(asset)
    feet = G.foot_plate_rows(asset)
    for flags, tag in ((0, "solo1"), (G.FRIC, "solo1-fric")):
        ref = G.reference("solo", asset, N, substeps=1, flags=flags)
        out = _step(_hip(ref, kernel, monkeypatch), ref)
        bad = _compare(tag, ref, kernel, out)
        k = ref.kept
        cf = out["cf"].reshape(N, -1, 3)
        loaded = B.loaded_rows(cf, asset)
        want = G.active_bodies(ref.terms, asset)
        allowed = np.zeros_like(loaded)
        allowed[np.arange(N), pb[ref.aim]] = True
        assert not (loaded & ~allowed).any(), np.flatnonzero((loaded & ~allowed).any(1))
        if asset == "cleats":
            assert not cf[:, feet].any()
        # (the fused step ends with the feet-sensor noise filter, which zeroes in place the components of the two foot rows of the
        # assets without cleats that do not exceed 0.01 N: there a foot row may be empty where the force is within the gate)
        o_rows = ref.out64["cf"].reshape(N, -1, 3)
        f = np.maximum(np.abs(cf[:, :nb]).max((1, 2)), np.abs(o_rows[:, :nb]).max((1, 2)))
        differ = k & ~bad & (loaded != want[:, :nb]).any(1)
        assert (f[differ] <= S.BARS["cf"][0]).all(), (np.flatnonzero(differ), f[differ])
        assert (np.abs(cf[k, nb]).max(1) > 0).all()
        assert loaded.any(1).mean() >= 0.85
        if flags == 0:
            assert not cf[:, :, 0:2].any()
        else:
            assert (np.abs(cf[loaded.any(1), :nb, 0:2]).max((1, 2)) > 0).mean() >= 0.95


@pytest.mark.parametrize("substeps", [1, 2, 3, 4, "3-last-fric"])
@pytest.mark.parametrize("kernel", KERNELS)
def test_substeps(kernel, substeps, monkeypatch):
    """The robot lying on the ground under gravity with at least two bodies loaded, at one to four substeps with the rows' mean over the
    substeps, and once more at three with BEZ_FLAG_CF_LAST_SUBSTEP | BEZ_FLAG_CF_WITH_FRICTION against the oracle with the same flags."""
    if substeps == "3-last-fric":
        ref = G.reference("lying", "default", N, substeps=3, flags=G.LAST | G.FRIC)
    else:
        ref = G.reference("lying", "default", N, substeps=substeps)
    _compare("lying-s%s" % substeps, ref, kernel, _step(_hip(ref, kernel, monkeypatch), ref))


@pytest.mark.parametrize("asset", ASSETS)
@pytest.mark.parametrize("kernel", KERNELS)
def test_lying(kernel, asset, monkeypatch):
    """On the front, the back and both sides within 0.25 rad, joints default +- 1 rad: torso + head, torso + forearm and head + forearm
    alone in at least 130 envs each, three or more of torso / head / forearms / feet in 51 - 62, every point under the plane in at least 30."""
    ref = G.reference("lying", asset, N)
    _compare("lying", ref, kernel, _step(_hip(ref, kernel, monkeypatch), ref))


@pytest.mark.parametrize("kernel", KERNELS)
def test_torso_row_sums_ball_and_ground(kernel, monkeypatch):
    """Lying on the front or back with a torso point under the plane and the ball pressed into the torso box from above: the torso row
    holds the ground force and the ball's in one store."""
    ref = G.reference("torso_ball", "default", 200)
    out = _step(_hip(ref, kernel, monkeypatch), ref)
    _compare("torso_ball", ref, kernel, out, p99=False)
    cf = out["cf"].reshape(ref.n, -1, 3)
    assert (np.abs(cf[:, 0]).max(1) > 0).mean() >= 0.5
    assert (np.abs(cf[:, B.ball_row("default")]).max(1) > 0).mean() >= 0.5


@pytest.mark.parametrize("kernel", KERNELS)
def test_contact_parameters(kernel, monkeypatch):
    """The free states with ground_contact_ref.PARAMS in the config of oracle and sim alike: every constant the contact law reads is
    off its default, the ball has its own spring and damper, and the slow envs split between the capped friction regime and the one
    inside veps under the cap."""
    ref = G.reference("free", "default", N, contact=G.PARAMS)
    _compare("free-params", ref, kernel, _step(_hip(ref, kernel, monkeypatch), ref))


@pytest.mark.parametrize("kernel", KERNELS)
def test_contact_free_neighbours(kernel, monkeypatch):
    """Sim A: every env with a ground contact of the robot and of the ball.  Sim B: the same states with robot and ball lifted 0.5 m
    clear of the ground everywhere except the first and last lanes of the 16- and 64-env workgroups and the last env.  Those envs agree
    between A and B bit for bit, and both meet the bars on all their envs.  (The p99 ratio is printed and reported here, not asserted:
    of 200 envs it is the third-worst env, for the reason measured in tests/test_gpu_leg_contact.py test_contact_free_neighbours.)"""
    n = 200
    dense, sparse = G.reference("free", "default", n), G.reference("sparse", "default", n)
    a, b = _hip(dense, kernel, monkeypatch), _hip(sparse, kernel, monkeypatch)
    oa, ob = _step(a, dense), _step(b, sparse)
    envs = list(S.NEIGHBOUR_ENVS)
    np.testing.assert_array_equal(np.flatnonzero((sparse.terms["d"] > 0).any(1)), envs)
    for name in ("root_states", "dof_state", "contact_forces"):
        x, y = getattr(a, name).reshape(n, -1), getattr(b, name).reshape(n, -1)
        np.testing.assert_array_equal(x[envs].view(np.uint32), y[envs].view(np.uint32), err_msg=name)
    away = np.ones(n, bool); away[envs] = False
    assert not ob["cf"][away].any()
    assert sparse.kept.all()
    _compare("sparse", sparse, kernel, ob, p99=False)
    _compare("dense200", dense, kernel, oa, p99=False)


@pytest.mark.parametrize("kernel", KERNELS)
def test_momentum(kernel, monkeypatch):
    """One substep in zero gravity with the friction in the rows: the change of the robot's linear momentum less dt x the sum of its
    rows, and of its angular momentum about its centre of mass less dt x the moment of that sum about it, is the integrator's own
    error, which the oracle shows in both precisions.  The kernel may show 3 x the fp32 build's max and p99 (the leg suite's rule)."""
    ref = G.reference("solo", "default", N, substeps=1, flags=G.FRIC)
    g = _hip(ref, kernel, monkeypatch)
    before = S.robot_momentum(g, N, "default")
    out = _step(g, ref)
    res = G.momentum_residual(before, S.robot_momentum(g, N, "default"), ref.com, ref.point, out["cf"], "default", float(ref.cfg().dt))
    k = ref.kept
    for col, what in ((0, "linear kg m/s"), (1, "angular kg m^2/s")):
        h, c = res[k, col], ref.res32[k, col]
        text = "%-36s momentum residual %s: HIP max %.3e p99 %.3e | fp32 build max %.3e p99 %.3e" % (
            "solo1-fric default %s" % kernel, what, h.max(), np.quantile(h, 0.99), c.max(), np.quantile(c, 0.99))
        print(text); _note(text)
    for col in (0, 1):
        h, c = res[k, col], ref.res32[k, col]
        assert h.max() <= 3.0 * c.max() and np.quantile(h, 0.99) <= 3.0 * np.quantile(c, 0.99)


@pytest.mark.parametrize("kernel", KERNELS)
def test_dof_force_recording_and_lean_step_leave_the_step_unchanged(kernel, monkeypatch):
    """The robot lying on the ground.  BEZ_FLAG_DOF_FORCE selects the recording instantiations of the step kernels: root state, DOF
    state, contact rows, observations and reward stay bit for bit what the plain instantiations compute.  BEZ_FLAG_LEAN_STEP skips the
    stores of the contact rows: root state, DOF state, observations -- the feet flags obs[44:52] among them, computed from the in-kernel
    forces -- and reward stay bit for bit the same (a process's first observation is never lean: both sims are told it is their second)."""
    ref = G.reference("lying", "default", N)
    off, on = _hip(ref, kernel, monkeypatch), _hip(ref, kernel, monkeypatch, flags=abi.FLAG_DOF_FORCE)
    off.step(ref.actions); on.step(ref.actions)
    on.sim.refresh_actuator_tensors()
    assert np.abs(on.sim.actuator_tensor(abi.ACTUATOR_DOF_FORCE).cpu().numpy()).max() > 0   # the recording really ran
    for name in ("root_states", "dof_state", "contact_forces", "obs", "rew"):
        x, y = getattr(off, name), getattr(on, name)
        np.testing.assert_array_equal(x.view(np.uint32), y.view(np.uint32), err_msg=name)
    assert off.sim.health() == 0 and on.sim.health() == 0
    full, lean = _hip(ref, kernel, monkeypatch), _hip(ref, kernel, monkeypatch, flags=abi.FLAG_LEAN_STEP)
    stale = lean.contact_forces
    for g in (full, lean):
        g.set_obs_calls(1)
        g.step(ref.actions)
    for name in ("root_states", "dof_state", "obs", "rew"):
        x, y = getattr(full, name), getattr(lean, name)
        np.testing.assert_array_equal(x.view(np.uint32), y.view(np.uint32), err_msg=name)
    assert np.abs(full.obs[:, 44:52]).max() > 0
    if kernel != "lane":   # the lean step really ran: its rows were not stored (the one-env-per-lane kernel does not read the flag)
        np.testing.assert_array_equal(lean.contact_forces, stale)
    assert np.abs(full.contact_forces - stale).max() > 1.0
    assert full.sim.health() == 0 and lean.sim.health() == 0
