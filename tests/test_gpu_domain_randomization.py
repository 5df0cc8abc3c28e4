"""GPU: domain randomisation inside the simulator -- the device-side redraws against the oracle's, their shard invariance, the noise
kernel, and the observation noise added inside the step."""
import numpy as np
import pytest

from tests.gpu_util import _dr_cfg

pytestmark = pytest.mark.gpu


def test_device_side_domain_randomization_matches_oracle():
    """the redraw at reset time (vec_task.py:505-725 via kick_env.py:781-782) runs inside the simulator.
    Same keyed Philox draws in the oracle: randomize_buf, the reset flags and every uniform-derived array (friction buckets,
    Kp, Kd) bit-exact; Box-Muller arrays (limits, gravity) and the noise scalars to 2e-6 (libm vs device logf / cosf); and the
    physics of the randomised envs keeps the usual parity bars.  N is not a multiple of 1024 (the DR kernel's stride)."""
    from bez_isaacgym_amd import abi
    from oracle.bez_oracle import Oracle
    from tests.sim_adapter import SimAdapter
    n = 1500
    dr = _dr_cfg()
    o, g = Oracle(abi.default_config(n, seed=9, env_id_offset=4096)), SimAdapter(abi.default_config(n, seed=9, env_id_offset=4096))
    o.set_randomization(dr); g.set_randomization(dr)
    exact = (abi.PARAM_FRICTION, abi.PARAM_KP_SCALE, abi.PARAM_KD_SCALE)
    close = (abi.PARAM_DOF_LOWER, abi.PARAM_DOF_UPPER, abi.PARAM_GRAVITY)

    def compare():
        np.testing.assert_array_equal(g.randomize_buf, o.randomize_buf)
        for p in exact:
            np.testing.assert_array_equal(g.get_env_params(p), o.get_env_params(p))
        for p in close:
            np.testing.assert_allclose(g.get_env_params(p), o.get_env_params(p), rtol=2e-6, atol=2e-6)
        np.testing.assert_allclose(g.dr_noise, o.dr_noise, rtol=1e-6, atol=0)
    compare()
    np.testing.assert_array_equal(o.get_env_params(abi.PARAM_FRICTION), 1.0)   # frame 0 of a linear schedule: nothing randomised yet
    rng = np.random.default_rng(2)
    redraws, grav = 0, set()
    for t in range(60):
        g.set_root_states(o.root_states); g.set_dof_state(o.dof_state); g.set_contact_forces(o.contact_forces)
        g.set_targets(o.targets); g.set_reset(o.reset_buf); g.set_progress(o.progress_buf)
        for p in close:   # keep the 1-ulp differences of the Box-Muller arrays out of the physics comparison
            g.set_env_params(p, o.get_env_params(p))
        before = o.get_env_params(abi.PARAM_KP_SCALE).copy()
        act = rng.uniform(-1, 1, (n, 18)).astype(np.float32)
        o.step(act); g.step(act)
        compare()
        redraws += int((np.abs(o.get_env_params(abi.PARAM_KP_SCALE) - before).max(axis=1) > 0).sum())
        grav.add(tuple(np.round(o.get_env_params(abi.PARAM_GRAVITY)[0], 6)))
        do, dg = o.dof_state.reshape(n, 18, 2), g.dof_state.reshape(n, 18, 2)
        flipped = np.abs(dg[..., 0] - do[..., 0]).max(1) > 1.5e-3   # an env on the other side of a switch (counted below) may also fall a step earlier / later
        np.testing.assert_array_equal(g.reset_buf[~flipped], o.reset_buf[~flipped])
        # the physics under the redrawn parameters: the usual bars for all but a handful of knife-edge elements (a jittered joint
        # limit or a saturating drive within rounding of its switch: DESIGN.md 6 "knife edges"), which stay small
        eq, ev = np.abs(dg[..., 0] - do[..., 0]), np.abs(dg[..., 1] - do[..., 1])
        assert (eq < 1.5e-4).mean() > 0.999 and eq.max() < 0.5, (t, eq.max())   # (round 6: a speed-limit switch within rounding is a larger jump than a saturating drive's)
        assert (ev < 1.5e-2).mean() > 0.999, (t, ev.max())
    assert redraws > n // 4, redraws          # random actions: most envs fell and were redrawn at least once
    assert len(grav) >= 5, grav               # gravity refreshed every `frequency` frames in which some env reset
    f = o.get_env_params(abi.PARAM_FRICTION)
    assert f.min() < 0.9 and f.max() > 1.1    # schedule complete: the whole U(0.7, 1.3) range is reached
    assert o.dr_noise[3] == np.float32(0.02) and o.dr_noise[1] == np.float32(0.002)


def test_device_side_domain_randomization_is_shard_invariant():
    """the draws are keyed by the GLOBAL env id: two shards of 300 envs reproduce the arrays of one sim of 600"""
    from bez_isaacgym_amd import abi
    from tests.sim_adapter import SimAdapter
    dr = _dr_cfg(freq=1, sched=0)
    whole = SimAdapter(abi.default_config(600, seed=4))
    parts = [SimAdapter(abi.default_config(300, seed=4, env_id_offset=300 * k)) for k in range(2)]
    for x in [whole] + parts:
        x.set_randomization(dr)
    for p in (abi.PARAM_FRICTION, abi.PARAM_KP_SCALE, abi.PARAM_DOF_UPPER):
        np.testing.assert_array_equal(np.concatenate([x.get_env_params(p) for x in parts]), whole.get_env_params(p))


def test_dr_noise_kernel_statistics_and_schedule():
    """bez_sim_add_dr_noise = the gaussian additive noise lambda of vec_task.py:586-592 in one launch: mean / std follow the
    device-resident BEZ_TENSOR_DR_NOISE, draws differ between calls of different frames and between observation / action kind."""
    import torch
    from bez_isaacgym_amd import abi
    from tests.sim_adapter import SimAdapter
    n = 4096
    g = SimAdapter(abi.default_config(n, seed=1))
    g.set_randomization(_dr_cfg(freq=1, sched=0))
    x = torch.zeros(n * 54, device=g.dev)
    g.sim.add_dr_noise(x, 0)
    assert abs(float(x.mean())) < 2e-5 and abs(float(x.std()) - 0.002) < 2e-5           # observations: N(0, 0.002)
    a = torch.zeros(n * 18 + 3, device=g.dev)                                            # not a multiple of 4
    g.sim.add_dr_noise(a, 1)
    assert abs(float(a.std()) - 0.02) < 3e-4 and float(a[-3:].abs().min()) > 0
    k = torch.mean(((a - a.mean()) / a.std()) ** 4)
    assert abs(float(k) - 3.0) < 0.15                                                    # gaussian kurtosis
    b = torch.zeros_like(a)
    g.sim.add_dr_noise(b, 1)
    assert torch.equal(a, b)                 # same frame, same kind: the same stream (one call per step and kind)
    g.step(np.zeros((n, 18), np.float32))    # next frame
    c = torch.zeros_like(a)
    g.sim.add_dr_noise(c, 1)
    assert not torch.equal(a, c) and abs(float((a * c).mean())) < 2e-5


@pytest.mark.parametrize("kernel,n", [("ws8", 4096), ("ws8", 200), ("ws8q", 200), ("lane", 256)])
def test_observation_noise_inside_the_step_equals_the_separate_launch(kernel, n, monkeypatch):
    """BEZ_FLAG_OBS_NOISE_IN_STEP: the post-physics part writes the noisy observations itself (the noise rides on the kernel's
    copy-out).  Two simulators with the same seed and randomisation, one with the flag, one adding the noise with
    bez_sim_add_dr_noise after every step: bit-identical observations over 40 steps (resets, a partial last workgroup at n = 200),
    everything else identical too; the call on the observation tensor is a no-op with the flag, a real launch on any other tensor."""
    import torch
    from bez_isaacgym_amd import abi
    from tests.sim_adapter import SimAdapter
    monkeypatch.setenv("BEZ_SIM_KERNEL", kernel)
    cfg_a, cfg_b = abi.default_config(n, seed=9), abi.default_config(n, seed=9)
    cfg_a.flags |= abi.FLAG_OBS_NOISE_IN_STEP
    a, b = SimAdapter(cfg_a), SimAdapter(cfg_b)
    for g in (a, b):
        g.set_randomization(_dr_cfg(freq=5, sched=0))
    obs_a, obs_b = a.sim.tensor(abi.TENSOR_OBS), b.sim.tensor(abi.TENSOR_OBS)
    rng = np.random.default_rng(2)
    clean_differs = False
    for t in range(40):
        act = rng.uniform(-1, 1, (n, 18)).astype(np.float32)
        a.step(act); b.step(act)
        clean = obs_b.clone()
        a.sim.add_dr_noise(obs_a, 0)          # no-op: the kernel has added it
        b.sim.add_dr_noise(obs_b, 0)          # the separate launch
        assert torch.equal(obs_a, obs_b), (t, float((obs_a - obs_b).abs().max()))
        clean_differs |= not torch.equal(clean, obs_b)
        d = (obs_b - clean).flatten()
        assert abs(float(d.std()) - 0.002) < 2e-4 and abs(float(d.mean())) < 2e-4
    assert clean_differs
    np.testing.assert_array_equal(a.root_states, b.root_states)
    np.testing.assert_array_equal(a.rew, b.rew); np.testing.assert_array_equal(a.reset_buf, b.reset_buf)
    x = torch.zeros(n * 54, device=a.dev)
    a.sim.add_dr_noise(x, 0)
    assert float(x.std()) > 1e-3              # any other tensor still gets its noise
