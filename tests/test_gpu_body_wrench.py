"""The external wrenches of the fused step kernels (bez_sim_apply_body_forces), body by body, against the fp64 oracle:
ext_prepare_kernel's resolution at the call (LOCAL vectors, ENV points, default points, fixed bodies folded into their links, the ball's
own frame), the moment matrix M = sum p F^T with axial(E M) in every substep, the EXT instantiations of the ws8, ws8q and lane kernels
on the default, cleats and box assets, at 1 - 4 substeps, with per-env parameters, in flight, standing, lying, with a state set between
the call and the launch, without a ball row, with a welded torso, and beside unloaded envs in the workgroup (tests/body_wrench_ref.py).

Every case is ONE control step from generated states written into an fp64 Oracle, its fp32 build and two HIP sims that have both made
an empty call first (the EXT instantiations), one loaded and one not.  Envs in which a joint decision of the loaded or the unloaded
fp64 step, or a contact of the start state, is nearer its boundary than the measured knife-edge margins (joint_drive_ref.kept,
ball_contact_ref.kept, ground_contact_ref.kept; at most 14 of 1000, tests/test_body_wrench_cpu.py) are left out.  The others are held
  (a) to the project's single-step bars (tests/step_terms.BARS through case_bars) with tests.parity_util.EnvOutliers' default budget,
      per quantity the p99 of |HIP - f64| to 2.5 x the p99 of the oracle's own fp32 build + 1e-6, and
  (b) in their RESPONSE, loaded - unloaded of root velocity, joint rates, ball velocity and spin, to the oracle's: 3 x the fp32 build's
      worst response error + 2 ulp32, inside the same budget of 3 envs per case -- (a)'s bars sit two to four orders above the fp32
      error, (b)'s at three times it; every (body, mode) cell keeps more envs than the budget.
ACTUATOR_STATUS of the hard pushes is held to the fp64 oracle's decision words exactly.  The health word stays zero.

What the oracle's fp32 build shows on these states (CPU, worst over the kept envs; tests/test_body_wrench_cpu.py prints the table) and
the HIP kernels beside it (MI355X, the worst of ws8 / ws8q / lane, outside their outliers `o`; profiles/body_wrench_errors.txt has every
case and kernel).  rv: root velocity, qd: joint rates, spin: the ball's; step: |x - f64|, response: |(loaded - unloaded) - f64's|:
    case                            kept; o  step: fp32 build|HIP                    response: fp32 build|HIP (bar)
    flight-solo-s2-plain default    1000; 0  rv 9.5e-07|7.2e-07  qd 6.3e-07|6.3e-07  rv 9.5e-07|7.7e-07 (2.4e-06)  qd 1.2e-06|1.2e-06 (3.7e-06)  spin 3.8e-06|3.8e-06 (9.5e-06)
    flight-solo-s2-dr default       1000; 0  rv 9.5e-07|9.5e-07  qd 1.3e-06|1.3e-06  rv 9.5e-07|1.0e-06 (2.4e-06)  qd 2.4e-06|2.4e-06 (6.6e-06)  spin 3.8e-06|3.8e-06 (9.5e-06)
    flight-solo-s2-plain cleats     1000; 0  rv 5.8e-07|1.4e-06  qd 6.3e-07|6.3e-07  rv 5.8e-07|1.4e-06 (2.0e-06)  qd 1.2e-06|1.3e-06 (3.6e-06)  spin 3.8e-06|3.8e-06 (9.5e-06)
    flight-solo-s2-dr cleats        1000; 0  rv 8.3e-07|9.5e-07  qd 1.3e-06|1.3e-06  rv 8.0e-07|8.6e-07 (2.4e-06)  qd 2.4e-06|2.4e-06 (6.4e-06)  spin 3.8e-06|3.8e-06 (9.5e-06)
    flight-solo-s2-plain box        1000; 0  rv 9.5e-07|7.2e-07  qd 6.3e-07|6.3e-07  rv 9.5e-07|7.7e-07 (2.4e-06)  qd 1.2e-06|1.2e-06 (3.7e-06)  spin 3.8e-06|3.8e-06 (9.5e-06)
    flight-solo-s2-dr box           1000; 0  rv 9.5e-07|9.5e-07  qd 1.3e-06|1.3e-06  rv 9.5e-07|1.0e-06 (2.4e-06)  qd 2.4e-06|2.4e-06 (6.6e-06)  spin 3.8e-06|3.8e-06 (9.5e-06)
    flight-solo-s1-plain default    1000; 0  rv 7.2e-07|1.1e-06  qd 4.1e-08|4.3e-08  rv 7.2e-07|1.1e-06 (2.4e-06)  qd 4.3e-08|4.0e-08 (1.0e-07)  spin 3.8e-06|3.8e-06 (9.5e-06)
    flight-solo-s3-plain default    1000; 0  rv 5.8e-07|7.2e-07  qd 1.2e-06|1.2e-06  rv 6.4e-07|7.3e-07 (1.8e-06)  qd 2.4e-06|2.4e-06 (6.3e-06)  spin 3.8e-06|3.8e-06 (1.2e-05)
    flight-solo-s4-plain default    1000; 0  rv 8.3e-07|6.0e-07  qd 1.9e-06|1.9e-06  rv 7.7e-07|5.7e-07 (1.9e-06)  qd 3.0e-06|3.0e-06 (8.2e-06)  spin 5.7e-06|5.7e-06 (2.1e-05)
    flight-solo-s4-plain cleats     1000; 0  rv 5.4e-07|6.0e-07  qd 1.8e-06|1.8e-06  rv 5.9e-07|6.6e-07 (1.9e-06)  qd 3.0e-06|3.1e-06 (8.1e-06)  spin 3.8e-06|3.8e-06 (1.2e-05)
    flight-solo-hard default        999; 1   rv 1.1e-05|1.5e-05  qd 1.8e-05|2.8e-05  rv 1.1e-05|1.5e-05 (3.0e-05)  qd 1.8e-05|1.3e-05 (1.9e-05)  spin 1.5e-05|1.6e-05 (3.9e-05)
    stance-solo default             990; 0   rv 1.9e-04|3.7e-04  qd 1.6e-03|2.8e-03  rv 8.0e-04|3.3e-04 (5.8e-04)  qd 4.3e-03|2.8e-03 (4.2e-03)  spin 3.5e-04|2.8e-04 (4.6e-04)
    stance-solo cleats              991; 2   rv 3.5e-04|7.6e-04  qd 1.7e-03|3.6e-03  rv 5.7e-04|3.2e-04 (6.0e-04)  qd 2.2e-03|1.6e-03 (2.5e-03)  spin 9.0e-04|2.5e-04 (4.6e-04)
    lying-solo default              986; 1   rv 4.8e-04|5.0e-04  qd 1.5e-03|1.2e-03  rv 4.8e-04|5.0e-04 (7.4e-04)  qd 2.6e-03|2.4e-03 (2.9e-03)  spin 8.1e-06|6.4e-06 (1.9e-05)
    lying-solo cleats               986; 1   rv 7.6e-04|8.5e-04  qd 2.7e-03|6.5e-03  rv 7.2e-04|5.4e-04 (1.1e-03)  qd 3.4e-03|2.2e-03 (5.5e-03)  spin 5.4e-06|1.8e-06 (9.5e-06)
    flight-all default              1000; 0  rv 7.2e-07|1.4e-06  qd 6.3e-07|6.3e-07  rv 7.5e-07|1.4e-06 (2.5e-06)  qd 1.2e-06|1.2e-06 (3.6e-06)  spin 5.7e-06|5.7e-06 (1.5e-05)
    flight-stacked default          1000; 0  rv 8.3e-07|1.4e-06  qd 6.3e-07|6.3e-07  rv 8.9e-07|1.5e-06 (2.8e-06)  qd 1.2e-06|1.2e-06 (3.7e-06)  spin 3.8e-06|3.8e-06 (1.5e-05)
    flight-all cleats               1000; 0  rv 9.5e-07|1.2e-06  qd 6.3e-07|6.4e-07  rv 9.5e-07|1.2e-06 (2.5e-06)  qd 1.2e-06|1.2e-06 (3.7e-06)  spin 3.8e-06|3.8e-06 (1.5e-05)
    flight-stacked cleats           1000; 0  rv 9.5e-07|1.3e-06  qd 6.3e-07|6.3e-07  rv 9.7e-07|1.3e-06 (2.6e-06)  qd 1.2e-06|1.2e-06 (3.6e-06)  spin 5.7e-06|3.8e-06 (1.9e-05)
    flight-all box                  1000; 0  rv 7.2e-07|1.4e-06  qd 6.3e-07|6.3e-07  rv 7.5e-07|1.4e-06 (2.5e-06)  qd 1.2e-06|1.2e-06 (3.6e-06)  spin 5.7e-06|5.7e-06 (1.5e-05)
    flight-stacked box              1000; 0  rv 8.3e-07|1.4e-06  qd 6.3e-07|6.3e-07  rv 8.9e-07|1.5e-06 (2.8e-06)  qd 1.2e-06|1.2e-06 (3.7e-06)  spin 3.8e-06|3.8e-06 (1.5e-05)
    late-solo default               1000; 0  rv 1.1e-06|9.5e-07  qd 6.3e-07|6.3e-07  rv 1.0e-06|9.5e-07 (2.5e-06)  qd 1.2e-06|1.2e-06 (3.6e-06)  spin 3.8e-06|3.8e-06 (9.5e-06)
    flight-solo walk default        1000; 0  rv 9.5e-07|1.2e-06  qd 6.3e-07|6.3e-07  rv 9.6e-07|1.2e-06 (2.6e-06)  qd 1.2e-06|1.2e-06 (3.7e-06)  spin 0.0e+00|0.0e+00 (2.8e-45)
    flight-solo fixed-base default  1000; 0  rv 0.0e+00|0.0e+00  qd 6.3e-07|6.3e-07  rv 0.0e+00|0.0e+00 (2.8e-45)  qd 1.2e-06|1.2e-06 (3.4e-06)  spin 3.8e-06|3.8e-06 (9.5e-06)
    flight-sparse200 default        200; 0   rv 2.1e-07|2.2e-07  qd 6.3e-07|6.3e-07  rv 2.1e-07|2.4e-07 (6.0e-07)  qd 1.0e-06|1.0e-06 (1.8e-06)  spin 0.0e+00|0.0e+00 (3.8e-06)
No kernel departed from DESIGN 4.3c: at most 2 of a case's 3 outliers were used (standing on cleats), the responses sit at 0.5 - 2 x
the fp32 build's, and no kept env's status differed from the fp64 decision.

BEZ_BODY_WRENCH_REPORT=<file>: every case appends its kept / outlier counts, per quantity the worst and p99 of the HIP kernel and of
the fp32 build, per response quantity the bar and both builds' worst and p99 (profiles/body_wrench_errors.txt)."""
import numpy as np
import pytest
import torch

from bez_isaacgym_amd import abi
from tests import body_wrench_ref as W
from tests import joint_drive_ref as J
from tests import step_terms as S
from tests.step_terms import KERNELS

pytestmark = pytest.mark.gpu

ASSETS = list(S.ASSETS)
STATE = ("root_states", "dof_state", "contact_forces", "obs", "rew")


def _hip(ref, kernel, monkeypatch, flags=0):
    """a HIP sim of a case that has made the empty call: it launches the EXT instantiations from its first step on"""
    g = S.hip_sim(ref, kernel, monkeypatch, flags, inject=False)
    g.apply_body_forces()
    return g


def _note(text):
    S.note("BEZ_BODY_WRENCH_REPORT", text)


def _step(g, ref, loaded):
    """the case's order of calls on one sim -- state, calls, (late: the second state,) one control step; the health word must stay clear"""
    S.inject(g, ref.states.get("first", ref.states), ref.params)
    if loaded:
        for F, Tq, X, space in ref.calls:
            g.apply_body_forces(F, Tq, X, space)
    if "first" in ref.states:
        S.inject(g, ref.states, ref.params)
    return S.step_outputs(g, ref)


def _run(name, ref, kernel, monkeypatch, flags=0, p99=True):
    """both sims of a case stepped and compared -> (loaded sim, unloaded sim, loaded outputs, unloaded outputs, outlier mask)"""
    a, b = _hip(ref, kernel, monkeypatch, flags), _hip(ref, kernel, monkeypatch, flags)
    out, unl = _step(a, ref, True), _step(b, ref, False)

    def report(*args):
        _note(W.report_line("%s %s" % (name, kernel or "selected"), ref, *args))
    bad = W.compare(name, ref, out, unl, kernel or "selected", report=report, p99=p99)
    return a, b, out, unl, bad


@pytest.mark.parametrize("dr", [False, True], ids=["plain", "dr"])
@pytest.mark.parametrize("asset", ASSETS)
@pytest.mark.parametrize("kernel", KERNELS)
def test_body_by_body(kernel, asset, dr, monkeypatch):
    """Flight, two substeps, env e loads body e % rows alone in mode (e // rows) % 4 of ENV / LOCAL x centre (force + torque) / point:
    88 cells on the default and box assets, 120 with cleats.  dr: per-env friction, Kp, Kd and mass scales."""
    name = "flight-solo-s2-%s %s" % ("dr" if dr else "plain", asset)
    _run(name, W.reference(**W.CASES[name]), kernel, monkeypatch)


@pytest.mark.parametrize("substeps,asset", [(1, "default"), (2, "default"), (3, "default"), (4, "default"), (4, "cleats")])
@pytest.mark.parametrize("kernel", KERNELS)
def test_substeps(kernel, substeps, asset, monkeypatch):
    """Flight, solo, at one to four substeps: from the second substep on the link frame (and the spinning ball's) is no longer the frame at
    the call -- the force stays fixed in world axes, the point moves with its body"""
    name = "flight-solo-s%d-plain %s" % (substeps, asset)
    _run(name, W.reference(**W.CASES[name]), kernel, monkeypatch)


def _actuator_status(g):
    g.sim.refresh_actuator_tensors()
    torch.cuda.synchronize()
    return g.sim.actuator_tensor(abi.ACTUATOR_STATUS).detach().cpu().numpy().reshape(g.n, 18).copy()


@pytest.mark.parametrize("kernel", KERNELS)
def test_pushes_that_lock_and_saturate(kernel, monkeypatch):
    """Flight, solo, pushes 10 - 20 times the easy ones with BEZ_FLAG_DOF_FORCE on: the wrench is in pA, so the held-parent predictors see
    it.  ACTUATOR_STATUS of every kept env equals the OR over the substeps of the fp64 oracle's decision word, exactly -- in the loaded
    sim and in the unloaded one -- and the loaded words show bits the unloaded ones do not."""
    name = "flight-solo-hard default"
    ref = W.reference(**W.CASES[name])
    a, b, _, _, _ = _run(name, ref, kernel, monkeypatch, flags=abi.FLAG_DOF_FORCE)
    k = ref.kept
    want, want_unl = (np.bitwise_or.reduce(w & J.STATUS_BITS, axis=1) for w in (ref.words64, ref.words64_unl))
    got, got_unl = _actuator_status(a), _actuator_status(b)
    assert (want[k] != want_unl[k]).any(1).mean() >= 0.10
    line = "%-44s status: kept envs whose status differs from the fp64 decision: loaded %d, unloaded %d; new bits in %d kept envs" % (
        "%s %s" % (name, kernel), (got != want).any(1)[k].sum(), (got_unl != want_unl).any(1)[k].sum(), W.new_bits(ref)[k].sum())
    print(line); _note(line)
    np.testing.assert_array_equal(got[k], want[k])
    np.testing.assert_array_equal(got_unl[k], want_unl[k])


@pytest.mark.parametrize("asset", ["default", "cleats"])
@pytest.mark.parametrize("scenario", ["stance", "lying"])
@pytest.mark.parametrize("kernel", KERNELS)
def test_on_the_ground(kernel, scenario, asset, monkeypatch):
    """Under gravity: standing on the feet (on the cleats with the cleats asset) with the ball against a foot or leg box, and lying with
    torso / head / forearm points under the plane; solo.  The contact rows are held to the cf bar against the oracle, whose rows are
    contact-only by construction; and in a kept env whose loaded body has no contact in either fp64 step, that body's row is its unloaded
    twin's within the bar: nothing of the wrench shows in it."""
    name = "%s-solo %s" % (scenario, asset)
    ref = W.reference(**W.CASES[name])
    _, _, out, unl, bad = _run(name, ref, kernel, monkeypatch)
    nbe = ref.tables.nbe
    free = np.ones(ref.n, bool)   # the loaded body touches nothing in the fp64 step, loaded or not (a push can take a leg off the ball)
    for o64 in (ref.out64, ref.unl64):
        free &= np.abs(o64["cf"].reshape(ref.n, nbe, 3)[np.arange(ref.n), ref.body]).max(1) == 0
    e = np.flatnonzero(ref.kept & ~bad & free)
    assert len(e) > 0.25 * ref.n
    atol = S.case_bars(ref)["cf"][0]
    got, twin = (x["cf"].reshape(ref.n, nbe, 3)[e, ref.body[e]] for x in (out, unl))
    assert np.abs(got - twin).max() <= atol, (name, kernel, np.abs(got - twin).max())
    assert (np.abs(ref.out64["cf"]).max(1) > 1.0)[ref.kept].mean() > 0.9   # (the envs do stand or lie on something)


@pytest.mark.parametrize("asset", ASSETS)
@pytest.mark.parametrize("kernel", KERNELS)
def test_all_bodies_and_stacked_calls(kernel, asset, monkeypatch):
    """Flight.  all: every body of every env in one call with points -- several bodies of one link and several points on one link folded
    into one moment matrix.  stacked: three calls before one launch, ENV without points, LOCAL with points, ENV with points, each on a
    random third of the bodies and on /torso, /imu_link and /camera: calls add up, across spaces."""
    for pattern in ("all", "stacked"):
        name = "flight-%s %s" % (pattern, asset)
        _run(name, W.reference(**W.CASES[name]), kernel, monkeypatch)


@pytest.mark.parametrize("kernel", KERNELS)
def test_call_then_set_state(kernel, monkeypatch):
    """The call is made from a first state, then the state is set, then the step: points and LOCAL vectors were resolved at the call"""
    name = "late-solo default"
    _run(name, W.reference(**W.CASES[name]), kernel, monkeypatch)


@pytest.mark.parametrize("kernel", KERNELS)
def test_tasks_without_a_ball(kernel, monkeypatch):
    """bez_walk: the body tensors have no ball row, solo over the 21 robot rows"""
    name = "flight-solo walk default"
    ref = W.reference(**W.CASES[name])
    assert ref.tables.nbe == ref.tables.nb == 21
    a, _, _, _, _ = _run(name, ref, kernel, monkeypatch)
    assert a.nbe == 21 and a.nact == 1


def test_fixed_base(monkeypatch):
    """BEZ_FLAG_FIX_BASE on the kernel the library selects for it, solo: the joints respond as the oracle's, and a wrench on the welded
    torso's own rows (/torso, /imu_link) moves nothing -- the loaded sim's state equals the unloaded one's bit for bit there"""
    name = "flight-solo fixed-base default"
    ref = W.reference(**W.CASES[name])
    a, b, out, unl, _ = _run(name, ref, None, monkeypatch)
    robot = ref.body < ref.tables.nb
    torso = np.flatnonzero(robot & (ref.tables.link[np.minimum(ref.body, ref.tables.nb - 1)] == 0))
    assert len(torso) >= 80
    for key in ("root_states", "dof_state"):
        x, y = getattr(a, key).reshape(ref.n, -1), getattr(b, key).reshape(ref.n, -1)
        np.testing.assert_array_equal(x[torso].view(np.uint32), y[torso].view(np.uint32), err_msg=key)
    assert (out["root_vel"] == 0).all() and (np.abs(out["qd"] - unl["qd"]).max(1)[ref.kept & robot & (ref.body > 1)] > 0).all()


@pytest.mark.parametrize("kernel", KERNELS)
def test_loaded_neighbours(kernel, monkeypatch):
    """200 envs, wrenches pending only in the first and last lanes of the 16- and 64-env workgroups and in the last env.  Every other env
    is bit for bit the unloaded sim's: the pending word is per env, and a role clears only its own links.  After the launch nothing is
    pending: a following step from the same state equals the unloaded sim's bit for bit in every env."""
    name = "flight-sparse200 default"
    ref = W.reference(**W.CASES[name])
    a, b, out, unl, _ = _run(name, ref, kernel, monkeypatch, p99=False)
    envs = list(S.NEIGHBOUR_ENVS)
    others = np.ones(ref.n, bool); others[envs] = False
    for key in STATE:
        x, y = getattr(a, key).reshape(ref.n, -1), getattr(b, key).reshape(ref.n, -1)
        np.testing.assert_array_equal(x[others].view(np.uint32), y[others].view(np.uint32), err_msg=key)
    assert (np.abs(out["root_vel"][envs] - unl["root_vel"][envs]).max(1) > 1e-3).all()
    for g in (a, b):
        S.inject(g, ref.states, ref.params)
        g.step(ref.actions)
        assert g.sim.health() == 0
    for key in ("root_states", "dof_state", "contact_forces"):
        np.testing.assert_array_equal(getattr(a, key).view(np.uint32), getattr(b, key).view(np.uint32), err_msg="following step: " + key)
