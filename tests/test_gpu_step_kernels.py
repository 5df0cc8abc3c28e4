"""GPU: the fused step kernels (eight role waves, four lanes per env, one env per lane) against each other and the forms the step is
launched in: other substep counts, the lean step, free flight at full size and HIP-graph replay."""
import numpy as np
import pytest

from tests.gpu_util import _adapter

pytestmark = pytest.mark.gpu


@pytest.mark.gpu
@pytest.mark.parametrize("substeps", [1, 3, 4])
def test_lane_group_kernel_at_other_substep_counts(substeps, monkeypatch):
    """The lane-group kernel's hand-overs are ordered by sequence words that count substeps (leg <-> leg sums, link packages): the default
    yaml runs 2; 1, 3 and 4 substeps step like the one-lane kernel too (resynchronised every step, the usual bars and outlier bookkeeping)."""
    from tests.parity_util import EnvOutliers
    from tests.sim_cfg import make_cfg
    n = 120

    def cfg():
        c = make_cfg(n, seed=17)
        c.substeps = substeps
        return c
    a = _adapter(cfg(), "ws8", monkeypatch)
    b = _adapter(cfg(), "ws8q", monkeypatch)
    rng = np.random.default_rng(5)
    T = EnvOutliers(n)
    for t in range(25):
        b.set_root_states(a.root_states); b.set_dof_state(a.dof_state); b.set_contact_forces(a.contact_forces)
        b.set_targets(a.targets); b.set_reset(a.reset_buf); b.set_progress(a.progress_buf); b.set_prev_lin_vel(a.prev_lin_vel)
        act = rng.uniform(-1, 1, (n, 18)).astype(np.float32)
        a.step(act); b.step(act)
        np.testing.assert_array_equal(b.progress_buf, a.progress_buf)
        ra, rb = a.root_states, b.root_states
        assert np.isfinite(rb).all()
        T.close(rb[..., 0:7], ra[..., 0:7], 2e-5, what="pose")
        T.close(rb[..., 7:13], ra[..., 7:13], 4e-3, what="vel")
        da, db = a.dof_state.reshape(n, 18, 2), b.dof_state.reshape(n, 18, 2)
        T.close(db[..., 0], da[..., 0], 1e-4, what="q")
        T.close(db[..., 1], da[..., 1], 1.5e-2, what="qd")
        T.close(b.contact_forces, a.contact_forces, 2.5e-2, rtol=4e-3, what="cf")
        T.end_step()
    T.finish()


def test_lean_step_changes_nothing_the_rollout_reads():
    """BEZ_FLAG_LEAN_STEP: the fused step skips the stores of the contact-force rows, FEET and PREV_LIN_VEL (308 B / env-step).
    State, observations (incl. the feet flags, computed from the in-kernel forces), reward and bookkeeping stay bit-identical;
    the three tensors freeze at their last non-lean values."""
    from bez_isaacgym_amd import abi
    from tests.sim_adapter import SimAdapter
    n = 300
    a = SimAdapter(abi.default_config(n, seed=5))
    c = abi.default_config(n, seed=5); c.flags |= abi.FLAG_LEAN_STEP
    b = SimAdapter(c)
    rng = np.random.default_rng(1)
    frozen = None
    for t in range(40):
        act = rng.uniform(-1, 1, (n, 18)).astype(np.float32)
        a.step(act); b.step(act)
        np.testing.assert_array_equal(b.obs, a.obs)
        np.testing.assert_array_equal(b.rew, a.rew)
        np.testing.assert_array_equal(b.reset_buf, a.reset_buf); np.testing.assert_array_equal(b.progress_buf, a.progress_buf)
        np.testing.assert_array_equal(b.root_states, a.root_states); np.testing.assert_array_equal(b.dof_state, a.dof_state)
        np.testing.assert_array_equal(b.targets, a.targets)
        if t == 0:
            np.testing.assert_array_equal(b.contact_forces, a.contact_forces)   # the process's first step is never lean (prev_lin_vel is read back once)
            frozen = b.contact_forces
        else:
            np.testing.assert_array_equal(b.contact_forces, frozen)
    assert np.abs(a.contact_forces - frozen).max() > 1.0
    assert a.obs[:, 44:52].max() == 1.0 and a.obs[:, 44:52].min() == -1.0


@pytest.mark.parametrize("kernel", ["ws8", "ws8q", "lane"])
def test_free_flight_momentum_at_full_size(model, kernel, monkeypatch):
    """A size-independent property at BASELINE's full size (4096 envs) on the production kernel: in free flight (robot dropped from
    5 m, the ball parked far away) drives, joint friction and joint limits are INTERNAL forces -- whatever the 18 targets do, the
    robot's linear momentum changes by exactly M g t and its angular momentum about the centre of mass does not change.  The sums
    come from the Isaac-visible rigid-body rows (origin velocity, spin) and the URDF masses / inertias, i.e. independently of the
    kernel's own articulated-body quantities.  (Round 6: the speed limit itself is a constraint inside the ABA and reacts on the parent --
    tests/test_gpu_joint_limits.py holds that; here small actions keep the motion slow enough for the integrator's own drift to stay under the bar.)"""
    import torch
    from bez_isaacgym_amd import abi
    from tests.rbd_numpy import quat_to_mat
    from tests.sim_adapter import SimAdapter
    monkeypatch.setenv("BEZ_SIM_KERNEL", kernel)
    n = 4096
    cfg = abi.default_config(n, seed=11)
    g = SimAdapter(cfg)
    root = g.root_states.reshape(n, 2, 13).copy()
    root[:, 0, 2] = 5.0
    root[:, 1, 0:3] = [50.0, 50.0, 0.08]
    g.set_root_states(root.reshape(-1, 13))
    links = model["links"]
    mass = np.array([L["mass"] for L in links]); com = np.array([L["com"] for L in links]); body = np.array([L["body"] for L in links])
    inertia = np.array([[[L["inertia"][0], L["inertia"][3], L["inertia"][4]], [L["inertia"][3], L["inertia"][1], L["inertia"][5]],
                         [L["inertia"][4], L["inertia"][5], L["inertia"][2]]] for L in links])
    M = mass.sum()

    def momenta():
        rb = g.rigid_body_states.reshape(n, -1, 13).astype(np.float64)[:, body]            # (n, links, 13)
        q = rb[..., 3:7]
        x, y, z, w = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
        R = np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], -1),
                      np.stack([2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)], -1),
                      np.stack([2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], -1)], -2)
        assert np.allclose(R[0, 0], quat_to_mat(q[0, 0]), atol=1e-12)
        rc = np.einsum("nlij,lj->nli", R, com)
        pc = rb[..., 0:3] + rc                                      # link centres of mass
        vc = rb[..., 7:10] + np.cross(rb[..., 10:13], rc)
        p = (mass[None, :, None] * vc).sum(1)
        cm = (mass[None, :, None] * pc).sum(1) / M
        Iw = np.einsum("nlij,ljk,nlmk->nlim", R, inertia, R)
        L = (np.cross(pc - cm[:, None], mass[None, :, None] * vc) + np.einsum("nlij,nlj->nli", Iw, rb[..., 10:13])).sum(1)
        return p, L

    g.set_reset(np.zeros(n, np.int64))
    g.simulate()                                     # one step to leave the reset state behind (targets = default)
    p0, L0 = momenta()
    rng = np.random.default_rng(3)
    steps = 20
    qd_max = np.zeros(n)
    for t in range(steps):
        g.pre_physics(rng.uniform(-0.08, 0.08, (n, 18)).astype(np.float32))
        g.simulate()
        qd_max = np.maximum(qd_max, np.abs(g.dof_state.reshape(n, 18, 2)[:, :, 1]).max(1))
    p1, L1 = momenta()
    free = qd_max < 6.0                       # envs in which no joint came near the 2 pi rad/s limit
    assert free.mean() > 0.97, free.mean()
    t_s = steps * float(cfg.dt)
    want = np.array([0.0, 0.0, -9.81 * M * t_s])
    # fp32 state, 40 substeps: the momentum of a 2.83 kg robot falling at 3.3 m/s is 9.3 N s; measured error: median 1e-3 per step
    # Round 6: a third of the reset draws start with the leg capsules overlapping (+-0.15 rad on the hip rolls) and the -- now stiff --
    # leg<->leg contact throws the legs apart in the first steps: the integrator's O(h) drift of those envs is larger (the fp64 oracle
    # shows the same numbers, 0.12 at 2 substeps -> 0.003 at 8 -> 0.0008 at 32: it is the integrator's, tests/test_oracle_joint_limits.py)
    ep = np.abs((p1 - p0)[free] - want).max(1)
    dL = np.abs((L1 - L0)[free]).max()
    assert np.quantile(ep, 0.99) < 2e-2 and ep.max() < 0.3, (np.quantile(ep, 0.99), ep.max())
    assert dL < 2e-2, dL


@pytest.mark.parametrize("task", ["bez_walk", "bez_orient"])
def test_walk_goal_draw_advances_under_graph_replay(task):
    """the goal of bez_walk / bez_orient is drawn per reset call (walk_env.py:570-575).  A captured HIP
    graph replays kernel arguments verbatim, so the draw must come from device state: capture ONE fused step, replay it with all
    envs flagged for reset, and the goal must follow the oracle's call-counter sequence step by step."""
    import torch
    from bez_isaacgym_amd import abi
    from tests.sim_adapter import SimAdapter
    from tests.sim_cfg import make_cfg, oracle
    n = 96
    g = SimAdapter(make_cfg(n, task=task, seed=5))
    o = oracle(n, task=task, seed=5)
    act = torch.zeros(n * 18, device=g.dev)
    reset = g.sim.tensor(abi.TENSOR_RESET)
    zero = np.zeros((n, 18), np.float32)
    # two eager steps (as the PPO loop's warm-up), then capture
    for _ in range(2):
        reset.fill_(1); o.set_reset(np.ones(n, np.int64))
        g.sim.step(act); o.step(zero)
        np.testing.assert_array_equal(g.goal, o.goal)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        reset.fill_(1)
        g.sim.step(act)  # warm the stream
        torch.cuda.synchronize()
        with torch.cuda.graph(graph, stream=side):
            g.sim.step(act)
    o.set_reset(np.ones(n, np.int64)); o.step(zero)   # the warm-up step above
    # NOTE: capture itself does not execute the step
    seen = []
    for k in range(6):
        reset.fill_(1); o.set_reset(np.ones(n, np.int64))
        graph.replay(); torch.cuda.synchronize()
        o.step(zero)
        gg = g.goal
        np.testing.assert_array_equal(gg, o.goal)      # bit-exact: same Philox draw, same counter
        assert (gg == gg[0]).all()                       # one draw per call, shared by every env it resets
        seen.append(tuple(gg[0]))
    assert len(set(seen)) == 6, seen                     # a fresh goal on every replay
