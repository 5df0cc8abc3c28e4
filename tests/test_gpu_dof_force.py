"""The DOF force tensor and actuator status (BEZ_FLAG_DOF_FORCE) on the GPU, on the three step kernels.

Measured on an MI355X (N m; the test prints them before it asserts), inverse-dynamics known answer of the first test:
    kernel  worst over all 1152 joints  worst on locked joints  p99 on the easy subset  oracle fp32 p99  ratio
    ws8     6.72e-6                     3.55e-7                 5.84e-6                 5.61e-6          1.04
    ws8q    6.72e-6                     3.58e-7                 5.84e-6                 5.61e-6          1.04
    lane    6.72e-6                     4.06e-7                 5.70e-6                 5.61e-6          1.02
(384 locked and 128 saturated joint samples, 768 in the subset.)"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from bez_isaacgym_amd import abi  # noqa: E402
from tests import dof_force_numpy as D  # noqa: E402
from tests import rbd_numpy as R  # noqa: E402
from tests.gpu_util import _adapter  # noqa: E402
from tests.scenarios import _free_space_cfg, _pressed_state   # noqa: E402

KERNELS = ["ws8", "ws8q", "lane"]


def _actuators(sim):
    sim.sim.refresh_actuator_tensors()
    torch.cuda.synchronize()
    n = sim.n
    return tuple(sim.sim.actuator_tensor(k).detach().cpu().numpy().reshape(n, 18).copy()
                 for k in (abi.ACTUATOR_DOF_FORCE, abi.ACTUATOR_DRIVE_TORQUE, abi.ACTUATOR_STATUS))


def test_flag_off_answers_an_error_not_zeros(monkeypatch):
    from bez_isaacgym_amd.sim import BezSimError
    sim = _adapter(abi.default_config(16), "ws8q", monkeypatch)
    assert sim.sim.lib.bez_sim_refresh_actuator_tensors(sim.sim.h, None) == -1
    assert b"BEZ_FLAG_DOF_FORCE" in sim.sim.lib.bez_sim_last_error(sim.sim.h)
    with pytest.raises(BezSimError):
        sim.sim.refresh_actuator_tensors()
    sim.sim.set_flags(int(sim.cfg.flags) | abi.FLAG_DOF_FORCE)   # accepted after creation: allocates
    sim.step(np.zeros((16, 18), np.float32))
    net, drive, status = _actuators(sim)
    assert np.isfinite(net).all() and np.abs(net).max() > 0


@pytest.mark.parametrize("kernel", KERNELS)
def test_dof_force_is_the_inverse_dynamics_torque_on_every_joint(model, kernel, monkeypatch):
    """Known answer without knowledge of the kernel's decisions: one substep in free space without leg <-> leg contact from 64 pressed
    states (several joints near the speed limit, saturated targets, hip rolls apart).  RNEA on the states read back before / after gives the
    joint torques; DOF_FORCE - armature * qdd equals them on ALL 18 joints of every env, locked and saturated ones included: 2e-2 N m.  On
    the easy subset (off the limit, PD inside 0.8 x effort) the p99 error is held to 2.5 x the p99 of the oracle's fp32 build stepped from
    the same states."""
    from tests.scenarios import make_backend
    n = 64
    cfg = _free_space_cfg(n, substeps=1)
    cfg.flags |= abi.FLAG_NO_SELF_COLLISION | abi.FLAG_DOF_FORCE
    sim = _adapter(cfg, kernel, monkeypatch)
    sim.step(np.zeros((n, 18), np.float32))
    acts = D.inject_pressed(sim, n, model, 21, _pressed_state)
    rs0 = sim.root_states.reshape(n, 2, 13).astype(np.float64); ds0 = sim.dof_state.reshape(n, 18, 2).astype(np.float64)
    sim.pre_physics(acts); sim.simulate()
    rs1 = sim.root_states.reshape(n, 2, 13).astype(np.float64); ds1 = sim.dof_state.reshape(n, 18, 2).astype(np.float64)
    net, drive, status = _actuators(sim)
    tau, qdd = D.rnea_torques(R, model, cfg, rs0, rs1, ds0, ds1)
    err = np.abs(net - float(cfg.armature) * qdd - tau)
    pd, _, _ = D.restate(cfg, model, ds0[:, :, 0], ds0[:, :, 1], ds1[:, :, 0], ds1[:, :, 1], sim.targets.reshape(n, 18))
    ok = D.easy_subset(cfg, pd, ds1[:, :, 1])
    # the oracle's fp32 build from the same states: the same error of the restated formula
    ocfg = _free_space_cfg(n, substeps=1); ocfg.flags |= abi.FLAG_NO_SELF_COLLISION
    orc = make_backend("oracle", ocfg, precision="f32")
    orc.step(np.zeros((n, 18), np.float32))
    orc.set_root_states(rs0.reshape(-1, 13).astype(np.float32)); orc.set_dof_state(ds0.reshape(-1, 2).astype(np.float32))
    o0r = orc.root_states.reshape(n, 2, 13).astype(np.float64); o0d = orc.dof_state.reshape(n, 18, 2).astype(np.float64)
    orc.pre_physics(acts); orc.simulate()
    o1r = orc.root_states.reshape(n, 2, 13).astype(np.float64); o1d = orc.dof_state.reshape(n, 18, 2).astype(np.float64)
    otau, oqdd = D.rnea_torques(R, model, ocfg, o0r, o1r, o0d, o1d)
    opd, onet, _ = D.restate(ocfg, model, o0d[:, :, 0], o0d[:, :, 1], o1d[:, :, 0], o1d[:, :, 1], orc.targets.reshape(n, 18))
    ook = D.easy_subset(ocfg, opd, o1d[:, :, 1])
    oerr = np.abs(onet - (otau + float(ocfg.armature) * oqdd))[ook]
    p99, op99 = float(np.percentile(err[ok], 99)), float(np.percentile(oerr, 99))
    locked = (status & abi.ACTUATOR_LOCKED) != 0; sat = (status & abi.ACTUATOR_SATURATED) != 0
    print("DOF_FORCE_LEVELS kernel=%s worst_all=%.3g worst_locked=%.3g p99_subset=%.3g oracle_f32_p99=%.3g oracle_f32_worst=%.3g ratio=%.2f "
          "subset=%d locked=%d saturated=%d" % (kernel, err.max(), err[locked].max() if locked.any() else 0.0, p99, op99, oerr.max(), p99 / op99,
                                                ok.sum(), locked.sum(), sat.sum()))
    assert ((locked.sum(1) >= 3) & (sat.sum(1) >= 1)).sum() >= n // 2                      # the sample is not trivial
    assert (np.abs(np.abs(ds1[:, :, 1][locked]) - float(cfg.vel_limit)) < 2e-4).all()      # locked by the status word = on the limit
    assert (np.abs(drive[sat]) == np.float32(cfg.effort)).all()
    assert err.max() < 2e-2, err.max()
    assert p99 <= 2.5 * op99, (p99, op99)


# Bar of the two equalities below: the issue sets "the tolerance measured in 1".  Test 1 measured 6.7e-6 N m; the PD law itself is evaluated
# here in fp64 from the fp32 read-back of q+ (a rounding of 2^-24 x |q| <= 1.2e-7 rad times kp x scale <= 130 N m/rad = 1.6e-5 N m at most),
# and this test measured 1.1e-5 (drive) and 3.1e-6 (friction + limit).  5e-5 N m: 3 x that rounding bound.
CONSISTENCY_BAR = 5e-5


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("dr", [False, True])
def test_internal_consistency_on_the_ground_with_a_push(model, kernel, dr, monkeypatch):
    """Gravity, ground contact, legs pressed together and an external push: status saturated => tau_drive == +-effort exactly; locked =>
    |qd+| == vel_limit within 2e-4; not saturated => tau_drive == kp (target - q+) - kd qd+; not locked => tau_net - tau_drive == the
    restated friction + limit terms (CONSISTENCY_BAR).  dr: per-env KP_SCALE / KD_SCALE / DOF_LOWER / DOF_UPPER (the DR instantiations,
    whose legs re-fetch them in front of pass 3), the limits drawn so that many joints start beyond them: a stale or unscaled gain or bound
    in the record shows here."""
    n = 64
    cfg = abi.default_config(n, seed=3); cfg.substeps = 1
    cfg.flags |= abi.FLAG_DOF_FORCE
    sim = _adapter(cfg, kernel, monkeypatch)
    sim.step(np.zeros((n, 18), np.float32))
    kps = kds = 1.0; lo = hi = None
    acts = D.inject_pressed(sim, n, model, 5, _pressed_state, hips_default=False)
    if dr:
        rng = np.random.default_rng(8)
        q0 = sim.dof_state.reshape(n, 18, 2)[:, :, 0]
        kps = rng.uniform(0.7, 1.3, (n, 18)).astype(np.float32); kds = rng.uniform(0.7, 1.3, (n, 18)).astype(np.float32)
        # a third of the joints start 0.02-0.1 rad below their per-env lower bound, a third above their upper bound
        pick = rng.integers(0, 3, (n, 18)); off = rng.uniform(0.02, 0.1, (n, 18))
        lo = np.where(pick == 0, q0 + off, np.asarray(model["dof_lower"], np.float32)[None]).astype(np.float32)
        hi = np.where(pick == 1, q0 - off, np.asarray(model["dof_upper"], np.float32)[None]).astype(np.float32)
        sim.set_env_params(abi.PARAM_KP_SCALE, kps); sim.set_env_params(abi.PARAM_KD_SCALE, kds)
        sim.set_env_params(abi.PARAM_DOF_LOWER, lo); sim.set_env_params(abi.PARAM_DOF_UPPER, hi)
        sim.set_env_params(abi.PARAM_FRICTION, rng.uniform(0.5, 1.2, (n, 1)).astype(np.float32))
    rs = sim.root_states.reshape(n, 2, 13).copy(); rs[:, 0, 2] = 0.34; rs[:, 0, 3:7] = (0, 0, 0, 1); rs[:, 0, 7:13] *= 0.1
    sim.set_root_states(rs.reshape(-1, 13))
    f = torch.zeros(n, sim.nbe, 3, device=sim.dev); f[:, 0, 0] = 5.0
    sim.sim.apply_body_forces(forces=f)
    ds0 = sim.dof_state.reshape(n, 18, 2).astype(np.float64)
    sim.pre_physics(acts); sim.simulate()
    ds1 = sim.dof_state.reshape(n, 18, 2).astype(np.float64)
    net, drive, status = _actuators(sim)
    pd, rnet, _ = D.restate(cfg, model, ds0[:, :, 0], ds0[:, :, 1], ds1[:, :, 0], ds1[:, :, 1], sim.targets.reshape(n, 18),
                            kp_scale=kps, kd_scale=kds, lower=lo, upper=hi)
    locked = (status & abi.ACTUATOR_LOCKED) != 0; sat = (status & abi.ACTUATOR_SATURATED) != 0
    assert locked.any() and sat.any()
    assert (drive[(status & abi.ACTUATOR_SATURATED_POS) != 0] == np.float32(cfg.effort)).all()
    assert (drive[(status & abi.ACTUATOR_SATURATED_NEG) != 0] == -np.float32(cfg.effort)).all()
    assert (np.abs(np.abs(ds1[:, :, 1][locked]) - float(cfg.vel_limit)) < 2e-4).all()
    assert (np.sign(ds1[:, :, 1][(status & abi.ACTUATOR_LOCKED_POS) != 0]) > 0).all()
    assert (np.sign(ds1[:, :, 1][(status & abi.ACTUATOR_LOCKED_NEG) != 0]) < 0).all()
    beyond = 0
    if dr:
        beyond = int((((ds0[:, :, 0] < lo) | (ds0[:, :, 0] > hi)) & ~locked).sum())
        assert beyond > n * 18 // 3          # the limit term is exercised on unlocked joints
    e1 = np.abs(drive - pd)[~sat].max(); e2 = np.abs((net - drive) - (rnet - pd))[~locked].max()
    print("DOF_FORCE_CONSISTENCY kernel=%s dr=%s drive_err=%.3g friction_limit_err=%.3g unsaturated=%d unlocked=%d beyond_limits=%d"
          % (kernel, dr, e1, e2, (~sat).sum(), (~locked).sum(), beyond))
    assert e1 < CONSISTENCY_BAR and e2 < CONSISTENCY_BAR, (e1, e2)


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("substeps", [2, 8])
def test_launch_reports_the_mean_over_its_substeps(model, kernel, substeps, monkeypatch):
    """substeps = S against the same states stepped as S launches of substeps = 1 with dt / S: the reported torques are the mean of the
    per-substep values and the status the OR (same kernel, same arithmetic: 1e-5 N m of summation order); step_many leaves the last step's
    values; a HIP-graph replay of step + refresh gives the eager values bit for bit."""
    n = 32
    def make(sub, dt):
        cfg = abi.default_config(n, seed=3); cfg.substeps = sub; cfg.dt = dt
        cfg.flags |= abi.FLAG_DOF_FORCE | abi.FLAG_CF_LAST_SUBSTEP
        s = _adapter(cfg, kernel, monkeypatch)
        s.step(np.zeros((n, 18), np.float32))
        return s
    dt = 0.01667
    a, b = make(substeps, dt), make(1, dt / substeps)
    acts = D.inject_pressed(a, n, model, 9, _pressed_state, hips_default=False)
    b.set_root_states(a.root_states.reshape(-1, 13)); b.set_dof_state(a.dof_state.reshape(-1, 2))
    a.pre_physics(acts); a.simulate()
    net, drive, status = _actuators(a)
    nets, drives, stats = [], [], []
    b.pre_physics(acts)
    for _ in range(substeps):
        b.simulate()
        x = _actuators(b); nets.append(x[0]); drives.append(x[1]); stats.append(x[2])
    np.testing.assert_array_equal(a.dof_state, b.dof_state)
    np.testing.assert_allclose(net, np.mean(nets, 0), atol=1e-5 * max(1.0, np.abs(net).max()))
    np.testing.assert_allclose(drive, np.mean(drives, 0), atol=1e-5)
    np.testing.assert_array_equal(status, np.bitwise_or.reduce(stats, 0))
    # step_many leaves the last step's values
    rng = np.random.default_rng(1)
    many = torch.as_tensor(rng.uniform(-1, 1, (3, n, 18)).astype(np.float32)).to(a.dev)
    c = make(substeps, dt)
    c.set_root_states(a.root_states.reshape(-1, 13)); c.set_dof_state(a.dof_state.reshape(-1, 2))
    a.sim.step_many(many.reshape(-1), 3); x_many = _actuators(a)
    for k in range(3):
        c.sim.step(many[k].reshape(-1).contiguous())
    x_single = _actuators(c)
    for u, v in zip(x_many, x_single):
        np.testing.assert_array_equal(u, v)
    # graph replay = eager, bit for bit
    act = many[0].reshape(-1).contiguous()
    c.set_root_states(a.root_states.reshape(-1, 13)); c.set_dof_state(a.dof_state.reshape(-1, 2))
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            c.sim.step(act); c.sim.refresh_actuator_tensors()
        g.replay()
    torch.cuda.synchronize()
    graph = tuple(c.sim.actuator_tensor(k).cpu().numpy().copy() for k in range(3))
    a.sim.step(act)
    eager = _actuators(a)
    for u, v in zip(graph, eager):
        np.testing.assert_array_equal(u.reshape(n, 18), v)


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("dr", [False, True])
def test_flag_on_changes_nothing_else(model, kernel, dr, monkeypatch):
    """300 random steps: state, obs, reward, reset, progress, contact rows and episode tensors are bit-identical with the flag on and off."""
    n, steps = 256, 300
    outs = []
    for flag in (0, abi.FLAG_DOF_FORCE):
        cfg = abi.default_config(n, seed=11); cfg.flags |= flag
        sim = _adapter(cfg, kernel, monkeypatch)
        if dr:
            rng = np.random.default_rng(2)
            sim.set_env_params(abi.PARAM_KP_SCALE, rng.uniform(0.7, 1.3, (n, 18)).astype(np.float32))
            sim.set_env_params(abi.PARAM_KD_SCALE, rng.uniform(0.7, 1.3, (n, 18)).astype(np.float32))
            sim.set_env_params(abi.PARAM_FRICTION, rng.uniform(0.5, 1.2, (n, 1)).astype(np.float32))
            sim.set_env_params(abi.PARAM_DOF_LOWER, (np.asarray(model["dof_lower"]) + 0.05).astype(np.float32)[None].repeat(n, 0))
        g = torch.Generator().manual_seed(4)
        acts = (torch.rand(steps, n, 18, generator=g) * 2 - 1).to(sim.dev)
        trace = []
        for k in range(steps):
            sim.sim.step(acts[k].reshape(-1).contiguous())
            if k % 50 == 49 or k == steps - 1:
                trace += [sim.root_states, sim.dof_state, sim.obs, sim.rew, sim.reset_buf, sim.progress_buf, sim.contact_forces, sim.targets,
                          sim.sim.episode_tensor(abi.EPISODE_END_BITS).cpu().numpy().copy(),
                          sim.sim.episode_tensor(abi.EPISODE_END_COUNTS).cpu().numpy().copy()]
        outs.append(trace)
        if flag:
            net, drive, status = _actuators(sim)
            assert np.isfinite(net).all() and np.isfinite(drive).all() and (status & ~15 == 0).all()
    for u, v in zip(*outs):
        np.testing.assert_array_equal(u, v)


@pytest.mark.parametrize("kernel", KERNELS)
def test_standing_robot_loads_knees_and_ankles_and_feels_a_push(model, kernel, monkeypatch):
    """Default pose on the ground, zero actions, 120 steps: knee and ankle-pitch DOF_FORCE are non-zero and left / right symmetric within
    the rollout's own asymmetry (the joint angles'), no status bit set; a 5 N push on the torso changes the ankle-pitch torques in that
    launch only."""
    n = 16
    cfg = abi.default_config(n, seed=3); cfg.flags |= abi.FLAG_DOF_FORCE
    sim = _adapter(cfg, kernel, monkeypatch)
    dflt = np.asarray(model["dof_default"], np.float32)
    sim.step(np.zeros((n, 18), np.float32))
    ds = np.zeros((n, 18, 2), np.float32); ds[:, :, 0] = dflt
    sim.set_dof_state(ds.reshape(-1, 2))
    for _ in range(120):
        sim.pre_physics(np.zeros((n, 18), np.float32)); sim.simulate()
    net, drive, status = _actuators(sim)
    knee_l, knee_r, ank_l, ank_r = 7, 15, 8, 16
    assert (status == 0).all()
    assert np.abs(net[:, [knee_l, knee_r, ank_l, ank_r]]).min() > 1e-3
    q = sim.dof_state.reshape(n, 18, 2)[:, :, 0]
    asym = np.abs(q[:, 4:10] - q[:, 12:18]).max() + 1e-3
    for l, r in ((knee_l, knee_r), (ank_l, ank_r)):
        assert np.abs(net[:, l] - net[:, r]).max() <= float(cfg.kp) * asym + 0.05, (net[:, l], net[:, r])
    # a twin from the same state without the push: the push shows in the ankle-pitch torques of the pushed launch, with one sign on
    # both stance ankles of every env (the pushed direction); a third sim started from the pushed sim's state afterwards and never pushed
    # then gives the pushed sim's next launch bit for bit: the push acted in that launch only
    def twin():
        t = _adapter(cfg, kernel, monkeypatch)
        t.step(np.zeros((n, 18), np.float32))
        t.set_root_states(sim.root_states.reshape(-1, 13)); t.set_dof_state(sim.dof_state.reshape(-1, 2))
        return t
    zero = np.zeros((n, 18), np.float32)
    plain = twin()
    f = torch.zeros(n, sim.nbe, 3, device=sim.dev); f[:, 0, 0] = 5.0
    sim.sim.apply_body_forces(forces=f)
    sim.pre_physics(zero); sim.simulate()
    plain.pre_physics(zero); plain.simulate()
    d = _actuators(sim)[0][:, [ank_l, ank_r]] - _actuators(plain)[0][:, [ank_l, ank_r]]
    print("DOF_FORCE_PUSH kernel=%s ankle-pitch DOF_FORCE change under a 5 N push: min %.4g max %.4g N m" % (kernel, d.min(), d.max()))
    # the sign: the ankle-pitch axis is -y (model axis of links 9 / 17); a +x push on the torso, above the ankles, puts a +y moment on the
    # leg about the ankle, and the joint resists it with a -y moment on its parent side = a NEGATIVE torque about its own axis
    assert (d < -1e-3).all(), d
    later = twin()
    later.sim.apply_body_forces(forces=torch.zeros_like(f))   # (nothing pending: only the same kernel instantiations as the pushed sim's)
    sim.pre_physics(zero); sim.simulate()
    later.pre_physics(zero); later.simulate()
    for u, v in zip(_actuators(sim), _actuators(later)):
        np.testing.assert_array_equal(u, v)


def test_the_three_kernels_agree_on_identical_states(model, monkeypatch):
    """Identical seeded states (pressed, on the ground, substeps = 2), one launch on ws8, ws8q and lane.  Envs whose status words differ
    between two kernels took different branches (a predictor on its threshold): counted, capped at the parity policy's 1.5e-3 of the
    env-steps with a floor of 3 (tests/parity_util.py), and left out; everything else agrees to the joint-speed bar of
    test_fused_step_kernels_agree (tests/test_gpu_round2.py: 1.5e-2 rad/s) scaled by kd + h kp, the torque one rad/s of
    end-of-substep speed is worth in the PD law."""
    n = 256
    outs = {}
    for kernel in KERNELS:
        cfg = abi.default_config(n, seed=3); cfg.flags |= abi.FLAG_DOF_FORCE
        sim = _adapter(cfg, kernel, monkeypatch)
        sim.step(np.zeros((n, 18), np.float32))
        acts = D.inject_pressed(sim, n, model, 13, _pressed_state, hips_default=False)
        rs = sim.root_states.reshape(n, 2, 13).copy(); rs[:, 0, 2] = 0.34; rs[:, 0, 3:7] = (0, 0, 0, 1); rs[:, 0, 7:13] *= 0.1
        sim.set_root_states(rs.reshape(-1, 13))
        sim.pre_physics(acts); sim.simulate()
        outs[kernel] = _actuators(sim)
    h = float(cfg.dt) / cfg.substeps
    bar = 1.5e-2 * (float(cfg.kd) + h * float(cfg.kp))
    cap = max(3, int(1.5e-3 * n))
    for a, b in (("ws8", "ws8q"), ("ws8", "lane"), ("ws8q", "lane")):
        flips = (outs[a][2] != outs[b][2]).any(1)
        same = ~flips
        dn = np.abs(outs[a][0] - outs[b][0])[same].max(); dd = np.abs(outs[a][1] - outs[b][1])[same].max()
        print("DOF_FORCE_AGREE %s vs %s: branch-flip envs %d (cap %d), net %.3g drive %.3g N m (bar %.3g)" % (a, b, flips.sum(), cap, dn, dd, bar))
        assert flips.sum() <= cap, flips.sum()
        assert dn < bar and dd < bar, (dn, dd)


def _env_and_agent(on, n=256):
    from bez_isaacgym_amd.ppo.a2c_continuous import A2CAgent
    from bez_isaacgym_amd.utils.config import load_config
    from bez_isaacgym_amd.utils.rlgames_utils import RLGPUEnv, get_rlgames_env_creator
    cfg = load_config(["task=bez_kick", "num_envs=%d" % n, "headless=True"])
    cfg["task"]["seed"] = 42
    if on is not None:
        cfg["task"]["env"]["enableDofForceSensors"] = on
    venv = RLGPUEnv("rlgpu", n, env_creator=get_rlgames_env_creator(cfg["task"], "bez_kick", "cuda:0", "cuda:0", 0, True))
    params = cfg["train"]["params"]
    params["config"].update(minibatch_size=4 * n, save_frequency=0, save_best_after=10 ** 9)
    return venv.env, A2CAgent(params, venv, "cuda:0")


def test_vec_task_views_alias_the_library_and_ppo_reports_actuators(tmp_path, monkeypatch):
    """VecTask with env.enableDofForceSensors: the three (N, 18) views are the library's buffers (same pointers, filled by
    refresh_dof_force_tensor); a short training run has finite actuators/* scalars with shares in [0, 1]; with the key off the epoch rows
    carry exactly the keys they always had and the attributes raise with the key's name."""
    import json
    import os
    rows = {}
    for on in (None, True):   # None: the key absent, as in the shipped yaml
        env, agent = _env_and_agent(on)
        if on:
            s = env.sim
            for view, which in ((env.dof_force_tensor, abi.ACTUATOR_DOF_FORCE), (env.dof_drive_torque, abi.ACTUATOR_DRIVE_TORQUE),
                                (env.dof_status, abi.ACTUATOR_STATUS)):
                assert view.shape == (256, 18) and view.data_ptr() == s.actuator_tensor(which).data_ptr()
            env.step(torch.rand(256, 18, device=env.device) * 2 - 1)
            assert env.refresh_dof_force_tensor() is True
            torch.cuda.synchronize()
            assert env.dof_force_tensor.abs().max().item() > 0 and torch.isfinite(env.dof_drive_torque).all()
        else:
            for name in ("dof_force_tensor", "dof_drive_torque", "dof_status"):
                with pytest.raises(AttributeError, match="enableDofForceSensors"):
                    getattr(env, name)
                assert not hasattr(env, name)
        agent.obs = agent.env_reset()
        rows[on] = [agent.train_epoch() for _ in range(3)]
        agent.release_env()
    parent_keys = {"play_time", "update_time", "total_time", "kl", "a_loss", "c_loss", "lr", "nonfinite_resets", "sim_health", "episode_ends"}
    assert all(set(r) == parent_keys for r in rows[None]), set(rows[None][0]) ^ parent_keys
    assert all(set(r) == parent_keys | {"actuators"} for r in rows[True])
    from bez_isaacgym_amd.ppo.a2c_continuous import A2CAgent
    from bez_isaacgym_amd.utils.rlgames_utils import RLGPUAlgoObserver
    ob = RLGPUAlgoObserver(str(tmp_path))
    for r in rows[True]:
        a = r["actuators"]
        assert set(a) == set(A2CAgent.ACTUATOR_NAMES) and all(np.isfinite(v) for v in a.values()), a
        assert 0.0 <= a["saturated_share"] <= 1.0 and 0.0 <= a["locked_share"] <= 1.0 and a["mean_abs_drive_torque"] > 0 and a["mean_positive_power"] >= 0
        ob.add(dict(r, epoch=1, frame=1, mean_reward=float("nan")))
    ob.f.close()
    line = json.loads(open(os.path.join(str(tmp_path), "scalars.jsonl")).readline())
    assert all(("actuators/" + k) in line["scalars"] for k in A2CAgent.ACTUATOR_NAMES)


@pytest.mark.parametrize("flag", [abi.FLAG_ANKLE_STOP, abi.FLAG_ALL_GROUND_SHAPES])
def test_untested_scenario_variants_are_refused(flag, monkeypatch):
    """BEZ_FLAG_DOF_FORCE with the scenario harness's two contact variants: rc -5 with a message, at create and at set_flags"""
    from bez_isaacgym_amd.sim import BezSim, BezSimError
    cfg = abi.default_config(16); cfg.flags |= flag | abi.FLAG_DOF_FORCE
    with pytest.raises(BezSimError, match=r"\(-5\).*BEZ_FLAG_DOF_FORCE"):
        BezSim(cfg, 0)
    sim = _adapter(abi.default_config(16), "lane", monkeypatch)
    with pytest.raises(BezSimError, match=r"\(-5\)"):
        sim.sim.set_flags(int(sim.cfg.flags) | flag | abi.FLAG_DOF_FORCE)


@pytest.mark.parametrize("variant", ["fix_base", "cleats", "box"])
def test_other_assets_and_fix_base_keep_the_consistency(model, variant, monkeypatch):
    """FIX_BASE (lane kernel), the cleats and the box asset (ws8q): the internal consistency of the record on the ground, CONSISTENCY_BAR"""
    n = 64
    cfg = abi.default_config(n, seed=3); cfg.substeps = 1
    cfg.flags |= abi.FLAG_DOF_FORCE | {"fix_base": abi.FLAG_FIX_BASE, "cleats": abi.FLAG_CLEATS, "box": abi.FLAG_BOX_ASSET}[variant]
    sim = _adapter(cfg, "ws8q", monkeypatch)
    sim.step(np.zeros((n, 18), np.float32))
    acts = D.inject_pressed(sim, n, model, 5, _pressed_state, hips_default=False)
    rs = sim.root_states.reshape(n, 2, 13).copy(); rs[:, 0, 2] = 0.34; rs[:, 0, 3:7] = (0, 0, 0, 1); rs[:, 0, 7:13] = 0
    sim.set_root_states(rs.reshape(-1, 13))
    ds0 = sim.dof_state.reshape(n, 18, 2).astype(np.float64)
    sim.pre_physics(acts); sim.simulate()
    ds1 = sim.dof_state.reshape(n, 18, 2).astype(np.float64)
    net, drive, status = _actuators(sim)
    pd, rnet, _ = D.restate(cfg, model, ds0[:, :, 0], ds0[:, :, 1], ds1[:, :, 0], ds1[:, :, 1], sim.targets.reshape(n, 18))
    locked = (status & abi.ACTUATOR_LOCKED) != 0; sat = (status & abi.ACTUATOR_SATURATED) != 0
    assert locked.any() and sat.any()
    assert (np.abs(drive[sat]) == np.float32(cfg.effort)).all()
    assert (np.abs(np.abs(ds1[:, :, 1][locked]) - float(cfg.vel_limit)) < 2e-4).all()
    e1 = np.abs(drive - pd)[~sat].max(); e2 = np.abs((net - drive) - (rnet - pd))[~locked].max()
    print("DOF_FORCE_VARIANT %s drive_err=%.3g friction_limit_err=%.3g" % (variant, e1, e2))
    assert e1 < CONSISTENCY_BAR and e2 < CONSISTENCY_BAR, (e1, e2)
