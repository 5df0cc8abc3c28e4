"""GPU: the HIP path, called through the C ABI, against (a) the golden vectors produced by the reference's own
code and (b) the fp64 CPU oracle on identical seeded inputs, plus size-independent properties at the
BASELINE size N=4096."""
import numpy as np
import pytest
import torch

from bez_isaacgym_amd import abi
from tests import golden_checks as GC
from tests.gpu_util import _pair
from tests.parity_util import EnvOutliers

pytestmark = pytest.mark.gpu

# fp32 HIP kernel vs fp64 oracle after ONE control step (2 substeps) from an identical state.
# Stated tolerances (DESIGN.md "Parity") = 2-3x the worst error tools/gpu_probe.py observes (128 envs x 40 resynchronised
# steps; HIP / the oracle's own fp32 build against the fp64 oracle): root and ball pose 7.5e-6 / 6.2e-6, joint angles 5.5e-5 /
# 6.6e-5, root and ball velocity 1.5e-3 / 1.1e-3, joint speeds 6.4e-3 / 7.7e-3 (they reach the 6.28 rad/s clamp), contact
# forces 1.6e-2 / 1.1e-2 N, reward 2.4e-6 / 6.4e-6.
ROOT_POS_ATOL, POS_ATOL, ROOT_VEL_ATOL, VEL_ATOL = 2e-5, 1.5e-4, 4e-3, 1.5e-2


@pytest.fixture(scope="module")
def sim64():
    from tests.sim_adapter import SimAdapter
    return SimAdapter(num_envs=GC.N)


def test_golden_imu(sim64, golden): GC.check_imu(sim64, golden)
def test_golden_off_orn(sim64, golden): GC.check_off_orn(sim64, golden)
def test_golden_feet(sim64, golden): GC.check_feet(sim64, golden)
def test_golden_reward_normal(sim64, golden): GC.check_reward(sim64, golden, "normal")
def test_golden_reward_edge(sim64, golden): GC.check_reward(sim64, golden, "edge")
def test_golden_pre_physics(sim64, golden): GC.check_pre_physics(sim64, golden)
def test_golden_step_sequence(sim64, golden): GC.check_step_sequence(sim64, golden)


def test_reset_state_bit_exact():
    """Philox reset noise + clamp: integer / fp32 work, must agree bit for bit (kick_env.py:786-791)."""
    o, g = _pair(256, seed=1234, env_id_offset=1000)
    np.testing.assert_array_equal(o.dof_state, g.dof_state)
    np.testing.assert_array_equal(o.root_states, g.root_states)
    np.testing.assert_array_equal(o.targets, g.targets)
    ids = np.arange(0, 256, 3, dtype=np.int32)
    o.reset_idx(ids); g.reset_idx(ids)
    np.testing.assert_array_equal(o.dof_state, g.dof_state)


def _compare_state(o, g, T, scale=1.0):
    """T: tests.parity_util.EnvOutliers -- every env within the bars except a counted handful per test (switches within rounding)"""
    ro, rg = o.root_states.reshape(-1, 2, 13), g.root_states.reshape(-1, 2, 13)
    T.close(rg[:, :, 0:7], ro[:, :, 0:7], ROOT_POS_ATOL * scale, what="pose")
    T.close(rg[:, :, 7:13], ro[:, :, 7:13], ROOT_VEL_ATOL * scale, what="vel")
    do, dg = o.dof_state.reshape(-1, 18, 2), g.dof_state.reshape(-1, 18, 2)
    T.close(dg[:, :, 0], do[:, :, 0], POS_ATOL * scale, what="q")
    T.close(dg[:, :, 1], do[:, :, 1], VEL_ATOL * scale, what="qd")


def test_single_step_parity_resynced():
    """For 40 control steps: copy the oracle's state into the HIP sim, step both with the same random actions,
    compare everything the step produces.  Resyncing every step measures the per-step error, not chaos."""
    from oracle.bez_oracle import Oracle
    n = 128
    o, g = _pair(n, seed=7)
    o32 = Oracle(abi.default_config(n, seed=7), precision="f32")  # the same C source built in fp32: what plain fp32 rounding costs
    rng = np.random.default_rng(3)
    worst = {"hip": {}, "cpu32": {}}
    T = EnvOutliers(n)
    for t in range(40):
        for x in (g, o32):
            x.set_root_states(o.root_states); x.set_dof_state(o.dof_state)
            x.set_contact_forces(o.contact_forces); x.set_targets(o.targets)
            x.set_reset(o.reset_buf); x.set_progress(o.progress_buf)
        act = rng.uniform(-1, 1, (n, 18)).astype(np.float32)
        o.step(act); g.step(act); o32.step(act)
        for tag, x in (("hip", g), ("cpu32", o32)):
            for k, a, b in (("root", o.root_states, x.root_states), ("dof", o.dof_state, x.dof_state), ("rew", o.rew, x.rew)):
                worst[tag][k] = max(worst[tag].get(k, 0.0), float(np.quantile(np.abs(a - b).reshape(n, -1).max(1), 0.99)))   # p99 over the envs: the level, not a switch
        # envs that were reset this step restart from the (bit-exact) reset draw: still comparable
        _compare_state(o, g, T)
        np.testing.assert_array_equal(g.progress_buf, o.progress_buf)
        np.testing.assert_array_equal(g.timeout_buf, o.timeout_buf)
        T.close(g.obs[:, :36], o.obs[:, :36], VEL_ATOL, what="obs")
        T.close(g.obs[:, 36:44], o.obs[:, 36:44], VEL_ATOL, what="obs imu")
        T.close(g.rew, o.rew, 2e-5, what="rew")
        cf_o, cf_g = o.contact_forces.reshape(n, 22, 3), g.contact_forces.reshape(n, 22, 3)
        bad = T.close(cf_g, cf_o, 0.04, rtol=0.01, what="cf")
        bad |= T.marked()
        np.testing.assert_array_equal(g.reset_buf[~bad], o.reset_buf[~bad])
        # the feet flags are threshold functions of the contact force: compare where the oracle is not within
        # tolerance of a threshold (0.01 N noise gate, 1 N load gate)
        fo = cf_o[:, [12, 20]]
        safe = (np.abs(np.abs(fo) - 0.01) > 0.06).all(axis=(1, 2)) & (np.abs(fo[:, :, 2] - 1.0) > 0.08).all(axis=1) & ~bad
        np.testing.assert_array_equal(g.obs[safe, 44:52], o.obs[safe, 44:52])
        T.end_step()
    T.finish()
    # the HIP kernel must not be worse than a plain fp32 build of the oracle by more than its own scatter (a regression in the
    # kernel's numerics shows here long before it reaches the absolute tolerances)
    for k in worst["hip"]:
        assert worst["hip"][k] <= 2.5 * worst["cpu32"][k] + 1e-6, (k, worst)


def test_rollout_parity_free():
    """Unsynchronised 10-step rollout from the common reset state.  Contact makes trajectories sensitive to
    rounding, so the bound is statistical: 90% of the envs stay within 5e-3 of the oracle, all within 0.1."""
    n = 256
    o, g = _pair(n, seed=11)
    rng = np.random.default_rng(5)
    for t in range(10):
        act = rng.uniform(-0.3, 0.3, (n, 18)).astype(np.float32)
        o.step(act); g.step(act)
    ok = (o.progress_buf == 10) & (g.progress_buf == 10)
    assert ok.sum() > n // 2
    ro, rg = o.root_states.reshape(n, 2, 13)[ok], g.root_states.reshape(n, 2, 13)[ok]
    err = np.abs(rg[:, :, 0:7] - ro[:, :, 0:7]).max(axis=(1, 2))
    qerr = np.abs(g.dof_state.reshape(n, 18, 2)[ok, :, 0] - o.dof_state.reshape(n, 18, 2)[ok, :, 0]).max(axis=1)
    assert np.quantile(err, 0.9) < 5e-3 and err.max() < 0.1, (np.quantile(err, 0.9), err.max())
    assert np.quantile(qerr, 0.9) < 1e-2 and qerr.max() < 0.3, (np.quantile(qerr, 0.9), qerr.max())


def test_fused_equals_split():
    """bez_sim_step == bez_sim_pre_physics + bez_sim_simulate + bez_sim_post_physics.  The two are different
    kernel instantiations (the compiler may contract/schedule differently), so: resync every step, tight tolerance."""
    from tests.sim_adapter import SimAdapter
    n = 192
    a, b = SimAdapter(abi.default_config(n, seed=5)), SimAdapter(abi.default_config(n, seed=5))
    rng = np.random.default_rng(9)
    T = EnvOutliers(n)
    for t in range(25):
        b.set_root_states(a.root_states); b.set_dof_state(a.dof_state); b.set_contact_forces(a.contact_forces)
        b.set_targets(a.targets); b.set_reset(a.reset_buf); b.set_progress(a.progress_buf)
        act = rng.uniform(-1, 1, (n, 18)).astype(np.float32)
        a.step(act)
        b.pre_physics(act); b.simulate(); b.post_physics()
        for name in ("progress_buf", "timeout_buf", "targets"):
            np.testing.assert_array_equal(getattr(a, name), getattr(b, name), err_msg=name)
        _compare_state(a, b, T)  # two kernels in fp32 (fused 8-wave vs the lane kernel's split entry points): observed 6e-6 / 1.4e-3 / 4e-5 / 4.7e-3
        T.close(a.obs, b.obs, 5e-3, what="obs")
        bad = T.close(a.rew, b.rew, 5e-4, what="rew") | T.marked()
        np.testing.assert_array_equal(a.reset_buf[~bad], b.reset_buf[~bad])
        T.end_step()
    T.finish()


def test_deterministic_and_shard_invariant():
    """Same seed -> identical trajectories; env i of a sim with env_id_offset=k equals env i+k of an unsharded sim
    (reset noise is keyed by the GLOBAL env id: results do not depend on the GPU count)."""
    from tests.sim_adapter import SimAdapter
    full = SimAdapter(abi.default_config(256, seed=21))
    again = SimAdapter(abi.default_config(256, seed=21))
    shard = SimAdapter(abi.default_config(128, seed=21, env_id_offset=128))
    rng = np.random.default_rng(2)
    for t in range(60):
        act = rng.uniform(-1, 1, (256, 18)).astype(np.float32)
        full.step(act); again.step(act); shard.step(act[128:])
    np.testing.assert_array_equal(full.obs, again.obs)
    np.testing.assert_array_equal(full.root_states, again.root_states)
    np.testing.assert_array_equal(full.obs[128:], shard.obs)
    np.testing.assert_array_equal(full.rew[128:], shard.rew)
    np.testing.assert_array_equal(full.progress_buf[128:], shard.progress_buf)


def test_full_size_standing_and_reset_cycle():
    """N=4096, zero actions: >= 99% of the envs stand in the ready pose for the whole 900-step episode (a few reset
    draws stumble into the ball and end early: the oracle shows the same 16 of 4096), the weight rests on the feet,
    and the horizon reset fires."""
    from tests.sim_adapter import SimAdapter
    n = 4096
    g = SimAdapter(abi.default_config(n))
    act = torch.zeros(n * 18, device=g.dev)
    for t in range(899):
        g.sim.step(act)
    ok = (g.progress_buf == 899) & (g.reset_buf == 0)
    assert ok.mean() >= 0.99, ok.mean()
    rs = g.root_states.reshape(n, 2, 13)[ok]
    # (a third of the reset draws start with the leg capsules overlapping by up to 2 cm -- +-0.15 rad on the hip rolls, feet 8 mm apart in the
    # default pose; the leg<->leg contact separates them in the first steps, which moves the standing robot a few centimetres)
    assert np.all(np.abs(rs[:, 0, 2] - 0.3235) < 0.01) and np.all(np.linalg.norm(rs[:, 0, :2], axis=1) < 0.2)
    cf = g.contact_forces.reshape(n, 22, 3)[ok]
    np.testing.assert_allclose(cf[:, 12, 2] + cf[:, 20, 2], 2.827994 * 9.81, rtol=0.02)
    assert (g.timeout_buf[ok] == 0).all()
    g.sim.step(act)
    assert (g.reset_buf[ok] == 1).all() and (g.progress_buf[ok] == 900).all() and (g.rew[ok] == 0).all() and (g.timeout_buf[ok] == 1).all()
    g.sim.step(act)
    assert (g.reset_buf[ok] == 0).all() and (g.progress_buf[ok] == 0).all()


def test_full_size_random_rollout_properties():
    """N=4096 random actions, 300 steps: everything stays finite, the 2 pi rad/s speed limit holds for the joints the in-dynamics limit
    predicted (round 6: a prescribed-rate joint inside the ABA, no rate is clamped afterwards; a miss lasts one substep --
    tools/vlimit_probe.py: ~3.5 % of the samples under random actions), quaternions stay unit, resets happen and episode counters restart."""
    from tests.sim_adapter import SimAdapter
    n = 4096
    g = SimAdapter(abi.default_config(n))
    gen = torch.Generator(device=g.dev); gen.manual_seed(0)
    acts = torch.rand(300, n * 18, device=g.dev, generator=gen) * 2 - 1
    nres = 0
    for t in range(300):
        g.sim.step(acts[t])
        if t % 50 == 49:
            assert np.isfinite(g.obs).all() and np.isfinite(g.rew).all()
            nres += int(g.reset_buf.sum())
    rs, ds = g.root_states.reshape(n, 2, 13), g.dof_state.reshape(n, 18, 2)
    assert np.isfinite(rs).all() and np.isfinite(ds).all()
    qd = np.abs(ds[:, :, 1])
    assert (qd > 2 * np.pi * 1.02).mean() < 0.08 and (np.abs(qd - 2 * np.pi) < 1e-3).mean() > 0.1 and qd.max() < 8 * 2 * np.pi, ((qd > 2 * np.pi * 1.02).mean(), qd.max())
    np.testing.assert_allclose(np.linalg.norm(rs[:, :, 3:7], axis=2), 1.0, atol=1e-4)
    assert nres > 0 and g.progress_buf.max() < 300


def test_kickenv_surface():
    """The VecTask/KickEnv mirror: shapes, dtypes and bookkeeping of step()/reset() (vec_task.py:303-377)."""
    from bez_isaacgym_amd.utils.config import load_config
    from bez_isaacgym_amd.tasks import isaacgym_task_map
    cfg = load_config(["task=bez_kick", "num_envs=64", "headless=True"])
    task_cfg = cfg["task"]
    task_cfg["rl_device"] = "cuda:0"
    env = isaacgym_task_map["bez_kick"](cfg=task_cfg, sim_device="cuda:0", graphics_device_id=0, headless=True)
    assert env.num_envs == 64 and env.num_obs == 54 and env.num_acts == 18 and env.max_episode_length == 900
    assert env.observation_space.shape == (54,) and env.action_space.shape == (18,)
    obs = env.reset()
    assert obs["obs"].shape == (64, 54) and obs["obs"].dtype == torch.float32
    o, r, d, info = env.step(torch.rand(64, 18, device="cuda:0") * 2 - 1)
    assert r.shape == (64,) and r.dtype == torch.float32 and d.dtype == torch.int64 and info["time_outs"].dtype == torch.int64
    assert (env.progress_buf == 2).all()
    assert env.root_pos_bez.shape == (64, 3) and env.root_orient_bez.shape == (64, 4) and env.dof_pos_bez.shape == (64, 18)
    np.testing.assert_allclose(env.obs_buf[:, 0:18].cpu().numpy(), env.dof_pos_bez.cpu().numpy(), atol=0)
    env.reset_idx(torch.arange(0, 64, 2, device="cuda:0"))
    assert (env.progress_buf[0::2] == 0).all() and (env.progress_buf[1::2] == 2).all()


def test_domain_randomization_parity():
    """Config 5 path: per-env friction / gain / mass / gravity arrays (vec_task.py:505-725 -> bez_sim_set_env_params)
    change the HIP step exactly as they change the oracle's."""
    n = 128
    o, g = _pair(n, seed=3)
    rng = np.random.default_rng(8)
    params = {abi.PARAM_FRICTION: rng.uniform(0.7, 1.3, (n, 1)), abi.PARAM_KP_SCALE: rng.uniform(0.5, 1.5, (n, 18)),
              abi.PARAM_KD_SCALE: rng.uniform(0.5, 1.5, (n, 18)), abi.PARAM_MASS_SCALE: rng.uniform(0.5, 1.5, (n, 19)),
              abi.PARAM_GRAVITY: np.tile([[0.0, 0.0, -9.81]], (n, 1)) + rng.normal(0, 0.3, (n, 3))}
    for k, v in params.items():
        o.set_env_params(k, v.astype(np.float32)); g.set_env_params(k, v.astype(np.float32))
    base_o, base_g = _pair(n, seed=3)
    T = EnvOutliers(n)
    for t in range(12):
        g.set_root_states(o.root_states); g.set_dof_state(o.dof_state); g.set_contact_forces(o.contact_forces)
        g.set_targets(o.targets); g.set_reset(o.reset_buf); g.set_progress(o.progress_buf)
        act = rng.uniform(-1, 1, (n, 18)).astype(np.float32)
        o.step(act); g.step(act); base_o.step(act)
        _compare_state(o, g, T)
        bad = T.marked(); T.end_step()
        np.testing.assert_array_equal(g.reset_buf[~bad], o.reset_buf[~bad])
    T.finish()
    assert np.abs(o.dof_state - base_o.dof_state).max() > 1e-2  # the randomisation really changed the dynamics
    g.set_env_params(abi.PARAM_MASS_SCALE, None)  # back to defaults is accepted
    g.step(act)


def test_ppo_epochs_on_gpu():
    """The consumer loop end to end on the GPU: KickEnv (fused HIP step) -> rollout buffer -> GAE -> AMP PPO update."""
    from bez_isaacgym_amd.utils.config import load_config
    from bez_isaacgym_amd.utils.rlgames_utils import RLGPUEnv, get_rlgames_env_creator
    from bez_isaacgym_amd.ppo.a2c_continuous import A2CAgent
    cfg = load_config(["task=bez_kick", "num_envs=512", "headless=True"])
    cfg["task"]["seed"] = 42
    creator = get_rlgames_env_creator(cfg["task"], "bez_kick", "cuda:0", "cuda:0", 0, True)
    venv = RLGPUEnv("rlgpu", 512, env_creator=creator)
    params = cfg["train"]["params"]
    params["config"].update(minibatch_size=4096, save_frequency=0, save_best_after=10 ** 9)
    agent = A2CAgent(params, venv, "cuda:0")
    assert agent.batch_size == 512 * 32 and agent.num_minibatches == 4
    agent.obs = agent.env_reset()
    stats = [agent.train_epoch() for _ in range(3)]
    assert all(np.isfinite([s["kl"], s["a_loss"], s["c_loss"]]).all() for s in stats)
    assert agent.frame == 3 * 512 * 32 and len(agent.game_rewards) > 0
    assert all(torch.isfinite(p).all() for p in agent.model.parameters())


def test_kickenv_domain_randomization_runs():
    """BASELINE config 5 surface: task.randomize=True hands randomization_params (bez_kick.yaml:151-219) to the simulator
    (VecTask.apply_randomizations -> bez_sim_set_randomization): per-env friction / gain / limit arrays exist on the device,
    noise lambdas wrap actions and observations and read their std on the device, training data stays finite, and the env step
    is graph-safe (no host sync)."""
    from bez_isaacgym_amd.utils.config import load_config
    from bez_isaacgym_amd.tasks import isaacgym_task_map
    cfg = load_config(["task=bez_kick", "num_envs=256", "headless=True", "task.task.randomize=True"])
    task_cfg = cfg["task"]
    task_cfg["rl_device"] = "cuda:0"
    env = isaacgym_task_map["bez_kick"](cfg=task_cfg, sim_device="cuda:0", graphics_device_id=0, headless=True)
    assert env.randomize and env.graph_safe and not env.first_randomization
    f0 = env.sim.get_env_params(abi.PARAM_FRICTION)
    np.testing.assert_allclose(f0.cpu().numpy(), 1.0, atol=1e-6)   # linear schedule at frame 0: no randomisation yet (vec_task.py:560-566)
    env.reset()
    for t in range(80):
        obs, rew, done, info = env.step(torch.rand(256, 18, device="cuda:0") * 2 - 1)
    assert torch.isfinite(obs["obs"]).all() and torch.isfinite(rew).all()
    assert "observations" in env.dr_randomizations and "actions" in env.dr_randomizations
    assert env.sim.get_env_params(abi.PARAM_KP_SCALE).shape == (256, 18) and env.sim.get_env_params(abi.PARAM_DOF_LOWER).shape == (256, 18)
    assert int(env.randomize_buf.max()) == 81 and env.randomize_buf.data_ptr() == env.sim.tensor(abi.TENSOR_RANDOMIZE_BUF).data_ptr()
