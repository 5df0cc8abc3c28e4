"""Ball <-> box contact of the fused step kernels, box by box, against the fp64 oracle and the numpy sphere-box test of
tests/ball_contact_ref.py: every one of the eleven boxes and every hand-over between the box owners of the wave kernels (role 2 ->
X_CANDH, roles 4 / 5 -> X_CAND, the leg role's foot box -> X_CANDF, role 3 -> X_TORSO; bez_kernel_ws8.h load_cand_depths / cand_winner),
on the default, cleats and box assets, with and without per-env parameters, at 1 - 4 substeps (the deferred ball update), with
contact-free neighbours in the workgroup (the any-env-has-contact skip) and with the DOF-force recording on.

Every case is ONE control step from generated states written into an fp64 Oracle, its fp32 build and the HIP sim.  Envs whose deepest
box leads by less than 0.1 mm are left out (tests/ball_contact_ref.kept: either box may win within rounding); the others are held to
the project's single-step bars (tests/test_gpu_parity.py) with tests.parity_util.EnvOutliers' default budget, and per quantity the p99
of |HIP - f64| to 2.5 x the p99 of the oracle's own fp32 build + 1e-6.

The bars, and next to them what the oracle's fp32 build shows on these states (CPU, worst over the kept envs outside the same budget of
3 envs, over all cases of this file; tests/step_terms.case_bars raises a bar to 3 x that figure if it came within a factor 2 of it,
which it does in no case):
    pose 2e-5 (3.7e-6)   root velocity 4e-3 (3.2e-4)   ball velocity 4e-3 (5.0e-5)   ball spin 4e-3 (4.3e-4)   q 1.5e-4 (3.4e-5)
    qd 1.5e-2 (4.1e-3)   contact forces 0.04 + 1 % (2.9e-6 beyond the 1 %)   obs[36:44] 1.5e-2 (7.7e-4)   reward 2e-5 (9.1e-6)
(the fp32 build's plain worst, its own branch flips included, is in profiles/ball_contact_errors.txt: at four substeps one env of it
misses a contact force by 16 N, as one env of each kernel does; that is what the budget is for).

BEZ_BALL_CONTACT_REPORT=<file>: every case appends its kept / outlier counts and per quantity the worst and p99 of the HIP kernel and of
the fp32 build (profiles/ball_contact_errors.txt)."""
import numpy as np
import pytest

from bez_isaacgym_amd import abi
from tests import ball_contact_ref as B
from tests import step_terms as S
from tests.step_terms import KERNELS, N, hip_sim as _hip

pytestmark = pytest.mark.gpu

ASSETS = list(S.ASSETS)
NS = abi.FLAG_NO_SELF_COLLISION


def _compare(case, ref, kernel, out):
    """step_terms.compare with the case's line of the report (this suite's line has no raised= word)"""
    def report(err, outliers, bars):
        S.note("BEZ_BALL_CONTACT_REPORT", "  ".join(S.report_words("%s %s %s" % (case, ref.asset, kernel), 34, ref, err, outliers)))
    return S.compare("%s %s" % (case, ref.asset), ref, out, kernel, report=report)


def _step(g, ref):
    return S.step_outputs(g, ref, health=False)


@pytest.mark.parametrize("dr", [False, True], ids=["plain", "dr"])
@pytest.mark.parametrize("asset", ASSETS)
@pytest.mark.parametrize("kernel", KERNELS)
def test_box_by_box(kernel, asset, dr, monkeypatch):
    """Free space, every env with the ball in one of the eleven boxes (each box the deepest in >= 15 kept envs, another owner's
    candidate positive in 2 of 3 envs: tests/test_ball_contact_cpu.py).  plain: no per-env parameters; dr: per-env friction (it feeds
    the ball contact), Kp and Kd scales on both sides.  Linear momentum of robot + ball, from the rigid-body rows and the URDF masses:
    the step's semi-implicit integration does not keep it exactly, the fp64 oracle and its fp32 build both show up to 0.43 kg m/s (p99
    0.20) on these states against ball impulses of up to 1.8 kg m/s; the kernel may show 3 x that."""
    ref = B.reference("free", asset, N, dr=dr)
    g = _hip(ref, kernel, monkeypatch)
    before = B.robot_ball_momentum(g, N, asset)
    out = _step(g, ref)
    dp = B.momentum_change(before, B.robot_ball_momentum(g, N, asset))
    bad = _compare("free-%s" % ("dr" if dr else "plain"), ref, kernel, out)
    k = ref.kept & ~bad
    print("momentum change: HIP max %.3e p99 %.3e, fp32 build max %.3e p99 %.3e" % (dp[k].max(), np.quantile(dp[k], 0.99), ref.dp32[ref.kept].max(), np.quantile(ref.dp32[ref.kept], 0.99)))
    assert dp[k].max() <= 3.0 * ref.dp32[ref.kept].max() and np.quantile(dp[k], 0.99) <= 3.0 * np.quantile(ref.dp32[ref.kept], 0.99)


@pytest.mark.parametrize("dr", [False, True], ids=["plain", "dr"])
@pytest.mark.parametrize("asset", ASSETS)
@pytest.mark.parametrize("kernel", KERNELS)
def test_loaded_row_is_the_numpy_winner(kernel, asset, dr, monkeypatch):
    """One substep, no leg<->leg contact, no ground: in every kept env the one loaded robot row of the kernel's contact forces is the
    body of the numpy winner (none where the kernel rejects a separating contact, which it may only where the oracle's force is
    within the bar of zero), every other robot row is exactly zero, and the ball row is equal and opposite to 1e-4 N + 1e-5 relative."""
    ref = B.reference("free", asset, N, substeps=1, dr=dr, flags=NS)
    g = _hip(ref, kernel, monkeypatch)
    out = _step(g, ref)
    bad = _compare("free1-%s" % ("dr" if dr else "plain"), ref, kernel, out)
    k = ref.kept
    nb = B.ball_row(asset)
    cf = out["cf"].reshape(N, -1, 3)
    loaded = B.loaded_rows(cf, asset)
    want = B.winner_body(ref.depths, asset)
    assert (loaded.sum(1)[k] <= 1).all(), np.flatnonzero(k & (loaded.sum(1) > 1))
    hit = k & (loaded.sum(1) == 1)
    np.testing.assert_array_equal(loaded.argmax(1)[hit], want[hit])
    # (the fused step ends with the reference's feet-sensor noise filter, which zeroes in place the components of the two foot rows
    # of the assets without cleats that do not exceed 0.01 N -- oracle feet_no_cleats, kick_env.py:987-990: there the robot's row
    # may be zero where the ball's is within the gate)
    robot, ball = cf[:, :nb].sum(1), cf[:, nb]
    feet = [B.box_table(asset)[b]["body"] for b in (4, 9)]
    gated = (asset != "cleats") & np.isin(want, feet)[:, None] & (np.abs(ball) <= 0.01 + 1e-4) & (robot == 0)
    balanced = np.abs(ball + robot) <= 1e-4 + 1e-5 * np.abs(robot)
    assert (balanced | gated)[k].all(), (np.flatnonzero(k & ~(balanced | gated).all(1)), ball[k & ~(balanced | gated).all(1)])
    # the rejection is the oracle's: a row missing on one side only belongs to a force within the bar of zero
    o_loaded = B.loaded_rows(ref.out64["cf"], asset).any(1)
    differ = k & ~bad & (o_loaded != loaded.any(1))
    f = np.maximum(np.abs(cf[:, :nb]).max((1, 2)), np.abs(ref.out64["cf"].reshape(N, -1, 3)[:, :nb]).max((1, 2)))
    assert (f[differ] <= S.BARS["cf"][0]).all(), (np.flatnonzero(differ), f[differ])
    rejected = (~loaded.any(1))[k].mean()
    assert 0.02 <= rejected <= 0.15, rejected


@pytest.mark.parametrize("asset", ASSETS)
@pytest.mark.parametrize("kernel", KERNELS)
def test_kick_stance(kernel, asset, monkeypatch):
    """The reset state standing on the ground under gravity, the ball on the ground next to a foot: calf, ankle and foot boxes of both
    legs win (tests/test_ball_contact_cpu.py), next to foot <-> ground and ball <-> ground contact."""
    ref = B.reference("kick", asset, N)
    _compare("kick", ref, kernel, _step(_hip(ref, kernel, monkeypatch), ref))


@pytest.mark.parametrize("substeps", [1, 3, 4])
@pytest.mark.parametrize("kernel", KERNELS)
def test_substeps(kernel, substeps, monkeypatch):
    """The ball is integrated one barrier late, with the previous substep's flags: one, three and four substeps (two: test_box_by_box)."""
    ref = B.reference("free", "default", N, substeps=substeps)
    _compare("free-s%d" % substeps, ref, kernel, _step(_hip(ref, kernel, monkeypatch), ref))


@pytest.mark.parametrize("kernel", ["ws8", "ws8q"])
def test_contact_free_neighbours(kernel, monkeypatch):
    """A leg wave skips the winner's block unless one of its envs has a ball <-> leg contact.  Sim A: every env in contact.  Sim B: the
    same states with the ball parked away everywhere except the first and last lanes of the 16- and 64-env workgroups and the last env.
    Those envs agree between A and B bit for bit (per-env results do not depend on the neighbours: test_deterministic_and_shard_invariant),
    and B meets the oracle's bars on all its envs."""
    n = 200
    dense, sparse = B.reference("free", "default", n), B.reference("sparse", "default", n)
    a, b = _hip(dense, kernel, monkeypatch), _hip(sparse, kernel, monkeypatch)
    oa, ob = _step(a, dense), _step(b, sparse)
    envs = list(S.NEIGHBOUR_ENVS)
    assert (B.winner(sparse.depths)[envs] >= 0).all() and (B.winner(sparse.depths) >= 0).sum() == len(envs)
    for name in ("root_states", "dof_state", "contact_forces"):
        x, y = getattr(a, name).reshape(n, -1), getattr(b, name).reshape(n, -1)
        np.testing.assert_array_equal(x[envs].view(np.uint32), y[envs].view(np.uint32), err_msg=name)
    assert sparse.kept.all()
    _compare("sparse", sparse, kernel, ob)
    _compare("dense200", dense, kernel, oa)


@pytest.mark.parametrize("kernel", KERNELS)
def test_dof_force_recording_leaves_the_step_unchanged(kernel, monkeypatch):
    """BEZ_FLAG_DOF_FORCE selects the recording instantiations of the step kernels: under ball contact on every box they leave root
    state, DOF state, contact rows, observations and reward bit for bit what the plain instantiations compute."""
    ref = B.reference("free", "default", N)
    off, on = _hip(ref, kernel, monkeypatch), _hip(ref, kernel, monkeypatch, flags=abi.FLAG_DOF_FORCE)
    off.step(ref.actions); on.step(ref.actions)
    on.sim.refresh_actuator_tensors()
    assert np.abs(on.sim.actuator_tensor(abi.ACTUATOR_DOF_FORCE).cpu().numpy()).max() > 0   # the recording really ran
    for name in ("root_states", "dof_state", "contact_forces", "obs", "rew"):
        x, y = getattr(off, name), getattr(on, name)
        np.testing.assert_array_equal(x.view(np.uint32), y.view(np.uint32), err_msg=name)
