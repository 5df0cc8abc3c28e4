"""The joint terms of the fused step kernels, joint by joint, against the fp64 oracle: the implicit PD drive, the effort saturation
chosen by the held-parent predictor, joint friction with its velocity floor, the implicit limit spring beyond lo / hi (the model's or
the env's own bounds) and the speed-limit lock -- joint_terms / joint_scalar (bez_kernels.h) and their copies in the wave kernels
(bez_ws_common.inc, bez_ws_quad.inc, bez_kernel_ws8.h) --, every one of the 18 joints aimed at every regime (tests/joint_drive_ref.py:
limits, drive, friction, pressed), on the default, cleats and box assets, with and without per-env parameters, at 1 - 4 substeps, with
easy neighbours in the workgroup, and with the DOF-force recording on.

Every case is ONE control step from generated states written into an fp64 Oracle, its fp32 build and the HIP sim.  Envs in which a
decision quantity of some joint and substep is nearer its boundary than the measured knife-edge margin (joint_drive_ref.kept:
tau_drive 6.5e-4 N m from +-effort, v_pred 4.7e-4 rad/s from +-vel_limit, q 7e-7 rad from lo / hi, |qd| 6.7e-6 rad/s from jfric_veps;
at most 13 of 1000, tests/test_joint_drive_cpu.py) are left out; the others are held to the project's single-step bars
(tests/step_terms.BARS through case_bars) with tests.parity_util.EnvOutliers' default budget, per quantity the p99 of |HIP - f64| to
2.5 x the p99 of the oracle's own fp32 build + 1e-6, and per aimed joint the worst q and qd error of that joint over ALL its kept envs
to the q / qd bars.  ACTUATOR_STATUS is held to the fp64 oracle's decision words exactly.  The health word stays zero.

What the oracle's fp32 build shows on these states (CPU, worst / p99 over the kept envs; tests/test_joint_drive_cpu.py prints the table),
and the HIP kernels beside it (the worst of ws8 / ws8q / lane; profiles/joint_drive_errors.txt):
                          fp32 build                                                    HIP (MI355X)
    limits, plain         root velocity 1.3e-6 / 5.2e-7  q 2.4e-7  qd 6.2e-6 / 5.5e-6   root velocity 9.8e-7 / 5.4e-7  q 2.4e-7  qd 6.2e-6 / 5.6e-6
    limits, dr            root velocity 1.1e-6 / 6.0e-7  q 1.2e-7  qd 3.6e-6 / 2.7e-6   root velocity 1.1e-6 / 6.6e-7  q 1.2e-7  qd 3.2e-6 / 2.7e-6
    drive, plain          root velocity 9.5e-7 / 3.6e-7  q 2.4e-7  qd 2.0e-6 / 1.4e-6   root velocity 1.1e-6 / 3.9e-7  q 2.4e-7  qd 4.8e-6 / 1.4e-6
    drive, dr             root velocity 1.8e-6 / 3.6e-7  q 2.4e-7  qd 9.6e-6 / 1.9e-6   root velocity 1.8e-6 / 4.2e-7  q 2.4e-7  qd 6.0e-6 / 1.9e-6
    friction, plain       root velocity 2.4e-7 / 1.8e-7  q 1.2e-7  qd 6.3e-7 / 6.3e-7   root velocity 3.0e-7 / 1.8e-7  q 1.2e-7  qd 6.3e-7 / 6.3e-7
    pressed, 4 substeps   root velocity 1.2e-5 / 3.5e-6  q 4.2e-7  qd 1.2e-4 / 5.4e-5   root velocity 1.4e-5 / 4.6e-6  q 4.8e-7  qd 1.3e-4 / 7.8e-5
two to four orders below the bars, so the p99 ratio, the per-joint check and the exact status do the work.  No env of any case was an
outlier on any kernel, no kept env's status differed from the fp64 decision, and the actuator record's p99 stayed within 1.07 x the
fp32 build's (drive torque 1.4e-5 against 1.3e-5 N m at worst).

BEZ_JOINT_DRIVE_REPORT=<file>: every case appends its kept / outlier counts, per quantity the worst and p99 of the HIP kernel and of
the fp32 build, the worst aimed-joint errors, the raised bars and the kept envs per regime (profiles/joint_drive_errors.txt)."""
import numpy as np
import pytest
import torch

from bez_isaacgym_amd import abi
from tests import joint_drive_ref as J
from tests import step_terms as S
from tests.step_terms import KERNELS, N, hip_sim as _hip, step_outputs as _step

pytestmark = pytest.mark.gpu

ASSETS = list(J.ASSETS)


def _note(text):
    S.note("BEZ_JOINT_DRIVE_REPORT", text)


def _compare(case, ref, kernel, out, p99=True):
    def report(err, outliers, bars, joints):
        _note(J.report_line("%s %s %s" % (case, ref.asset, kernel), ref, err, outliers, bars, joints))
    return J.compare("%s %s" % (case, ref.asset), ref, out, kernel, report=report, p99=p99)


def _actuators(g):
    g.sim.refresh_actuator_tensors()
    torch.cuda.synchronize()
    return tuple(g.sim.actuator_tensor(k).detach().cpu().numpy().reshape(g.n, 18).copy()
                 for k in (abi.ACTUATOR_DOF_FORCE, abi.ACTUATOR_DRIVE_TORQUE, abi.ACTUATOR_STATUS))


@pytest.mark.parametrize("dr", [False, True], ids=["plain", "dr"])
@pytest.mark.parametrize("asset", ASSETS)
@pytest.mark.parametrize("scenario", ["limits", "drive", "friction"])
@pytest.mark.parametrize("kernel", KERNELS)
def test_joint_by_joint(kernel, scenario, asset, dr, monkeypatch):
    """Zero gravity, two substeps, env e with joint e % 18 aimed at one regime of the scenario, every other joint in the easy regime.
    plain: no per-env parameters (limits: the state itself beyond the model's limits); dr: per-env friction, Kp and Kd scales (limits:
    and per-env bounds, moved inside the posture for the aimed joint and off the model's for every other)."""
    ref = J.reference(scenario, asset, N, dr=dr)
    _compare("%s-%s" % (scenario, "dr" if dr else "plain"), ref, kernel, _step(_hip(ref, kernel, monkeypatch), ref))


@pytest.mark.parametrize("scenario,dr", [(s, dr) for s in ("limits", "drive", "friction") for dr in (False, True)] + [("pressed", False)],
                         ids=lambda v: v if isinstance(v, str) else ("dr" if v else "plain"))
@pytest.mark.parametrize("kernel", KERNELS)
def test_status_is_the_fp64_decision(kernel, scenario, dr, monkeypatch):
    """With BEZ_FLAG_DOF_FORCE: in every kept env ACTUATOR_STATUS of all 18 joints equals the OR over the substeps of the fp64 oracle's
    decision word (its four status bits), exactly; DRIVE_TORQUE and DOF_FORCE against the oracle's own record (the means over the
    substeps) per env, the p99 of |HIP - f64| at most 2.5 x the fp32 build's + 1e-6; outside the kept envs everything is finite."""
    ref = J.reference(scenario, "default", N, dr=dr)
    g = _hip(ref, kernel, monkeypatch, flags=abi.FLAG_DOF_FORCE)
    _step(g, ref)
    net, drive, status = _actuators(g)
    k = ref.kept
    assert np.isfinite(net).all() and np.isfinite(drive).all() and (status & ~J.STATUS_BITS == 0).all()
    want = np.bitwise_or.reduce(ref.words64 & J.STATUS_BITS, axis=1)
    flips = (status != want).any(1)
    name = "%s-%s default %s" % (scenario, "dr" if dr else "plain", kernel)
    lines = ["%-34s status: kept=%d/%d envs whose status differs from the fp64 decision: %d kept, %d not kept; bits set %s" % (
        name, k.sum(), ref.n, (flips & k).sum(), (flips & ~k).sum(), np.bincount(want[k].reshape(-1), minlength=16).tolist())]
    stats = {}
    for what, got, i in (("drive", drive, 0), ("net", net, 1)):
        h = np.abs(got - ref.act64[i]).max(1)[k]
        c = np.abs(ref.act32[i] - ref.act64[i]).max(1)[k]
        stats[what] = (float(np.quantile(h, 0.99)), float(np.quantile(c, 0.99)))
        lines.append("%-34s %-5s N m: HIP max %.2e p99 %.2e | fp32 build max %.2e p99 %.2e" % (name, what, h.max(), stats[what][0], c.max(), stats[what][1]))
    for text in lines:
        print(text); _note(text)
    np.testing.assert_array_equal(status[k], want[k])
    for what, (h, c) in stats.items():
        assert h <= 2.5 * c + 1e-6, (name, what, h, c)


@pytest.mark.parametrize("substeps", [1, 2, 3, 4])
@pytest.mark.parametrize("kernel", KERNELS)
def test_substeps(kernel, substeps, monkeypatch):
    """tests/scenarios._pressed_state standing on the ground under gravity, the hip rolls at the default pose: six leg joints per env
    near the lock with saturated drives, at one to four substeps."""
    ref = J.reference("pressed", "default", N, substeps=substeps)
    _compare("pressed-s%d" % substeps, ref, kernel, _step(_hip(ref, kernel, monkeypatch), ref))


@pytest.mark.parametrize("kernel", KERNELS)
def test_unaimed_neighbours(kernel, monkeypatch):
    """Sim A: the drive states with only the first and last lanes of the 16- and 64-env workgroups and the last env aimed (saturated or
    locked), every other env in the easy regime.  Sim B: the same states with nobody aimed.  The other envs agree between A and B bit
    for bit: a decision does not leak across lanes or quads.  Both meet the bars on all their envs."""
    n = 200
    some, none = J.reference("drive_sparse", "default", n), J.reference("drive_none", "default", n)
    envs = list(S.NEIGHBOUR_ENVS)
    np.testing.assert_array_equal(np.flatnonzero(some.aim >= 0), envs)
    others = np.ones(n, bool); others[envs] = False
    for key in ("root_states", "dof_state", "actions"):
        np.testing.assert_array_equal(some.states[key][others], none.states[key][others])
    assert ((some.words64[envs] & J.STATUS_BITS) != 0).any((1, 2)).all() and not (none.words64 & J.STATUS_BITS).any()
    a, b = _hip(some, kernel, monkeypatch), _hip(none, kernel, monkeypatch)
    oa, ob = _step(a, some), _step(b, none)
    for name in ("root_states", "dof_state", "contact_forces", "obs", "rew"):
        x, y = getattr(a, name).reshape(n, -1), getattr(b, name).reshape(n, -1)
        np.testing.assert_array_equal(x[others].view(np.uint32), y[others].view(np.uint32), err_msg=name)
    assert (oa["qd"][envs] != ob["qd"][envs]).any(1).all()
    _compare("drive_sparse200", some, kernel, oa, p99=False)
    _compare("drive_none200", none, kernel, ob, p99=False)


@pytest.mark.parametrize("kernel", KERNELS)
def test_dof_force_recording_leaves_the_step_unchanged(kernel, monkeypatch):
    """The drive states.  BEZ_FLAG_DOF_FORCE selects the recording instantiations of the step kernels: root state, DOF state, contact
    rows, observations and reward stay bit for bit what the plain instantiations compute."""
    ref = J.reference("drive", "default", N)
    off, on = _hip(ref, kernel, monkeypatch), _hip(ref, kernel, monkeypatch, flags=abi.FLAG_DOF_FORCE)
    off.step(ref.actions); on.step(ref.actions)
    net, _, status = _actuators(on)
    assert np.abs(net).max() > 0 and (status != 0).any()   # the recording really ran
    for name in ("root_states", "dof_state", "contact_forces", "obs", "rew"):
        x, y = getattr(off, name), getattr(on, name)
        np.testing.assert_array_equal(x.view(np.uint32), y.view(np.uint32), err_msg=name)
    assert off.sim.health() == 0 and on.sim.health() == 0
