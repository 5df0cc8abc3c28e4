"""External forces and torques on the rigid bodies (bez_sim_apply_body_forces, VecTask.apply_rigid_body_force_tensors /
apply_rigid_body_force_at_pos_tensors) on every step kernel: known answers from the independent numpy RNEA, once-then-cleared,
HIP-graph replay, the non-finite guard, and a push that moves the robot."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from bez_isaacgym_amd import abi  # noqa: E402
from tests import rbd_numpy as R  # noqa: E402

KERNELS = ["ws8", "ws8q", "lane"]


def _sim(cfg, kernel, monkeypatch):
    from tests.sim_adapter import SimAdapter
    monkeypatch.setenv("BEZ_SIM_KERNEL", kernel)
    return SimAdapter(cfg)


def _free_cfg(n):
    """free space: no gravity, no drives, no joint friction, one substep, no speed limit in reach"""
    cfg = abi.default_config(n, seed=3)
    cfg.gravity[:] = [0.0, 0.0, 0.0]
    cfg.substeps = 1
    cfg.kp = 0.0; cfg.kd = 0.0; cfg.joint_friction = 0.0
    cfg.vel_limit = 1.0e9
    cfg.flags |= abi.FLAG_NO_SELF_COLLISION   # (an implicit leg<->leg contact would answer the push as well: not free space)
    return cfg


def _rand_quat(rng):
    q = rng.normal(size=4)
    return q / np.linalg.norm(q)


def _inject_rest(sim, model, n, rng, pairs=True):
    """every env at rest at z = 1, joints near the default pose, the ball at rest in the air 3 m away; the two envs of a pair equal"""
    dflt = np.asarray(model["dof_default"], float)
    rs = np.zeros((n, 2, 13), np.float32)
    ds = np.zeros((n, 18, 2), np.float32)
    for e in range(0, n, 2 if pairs else 1):
        rows = [e, e + 1] if pairs else [e]
        q = dflt + rng.uniform(-0.1, 0.1, 18)
        rq, bq = _rand_quat(rng), _rand_quat(rng)
        for k in rows:
            rs[k, 0, 0:3] = (0.0, 0.0, 1.0); rs[k, 0, 3:7] = rq
            rs[k, 1, 0:3] = (3.0, 0.0, 1.0); rs[k, 1, 3:7] = bq
            ds[k, :, 0] = q
    sim.set_root_states(rs.reshape(-1, 13)); sim.set_dof_state(ds.reshape(-1, 2))


def _link_frames(model, root_quat, q):
    """world rotation of every link and its origin relative to the torso origin (forward kinematics of the model JSON)"""
    links = model["links"]
    E = [None] * len(links); r = [None] * len(links)
    E[0] = R.quat_to_mat(root_quat); r[0] = np.zeros(3)
    for i in range(1, len(links)):
        p = links[i]["parent"]
        r[i] = r[p] + E[p] @ np.array(links[i]["xyz"])
        E[i] = E[p] @ R.rot_axis(links[i]["axis"], q[i - 1])
    return E, r


def _residuals(model, root_quat, q, qdd, a0, arm, wrench):
    """RNEA of the measured accelerations with (and without) the applied external wrench.  wrench = (link, moment about the torso
    origin, force), world axes.  The floating base must need exactly the external wrench (base coordinates), every joint
    tau + armature qdd = the external wrench's generalised force a . (M_O - r_j x F) on the joints that carry the link."""
    f0, tau = R.rnea_floating(model, root_quat, np.zeros(6), a0, q, np.zeros(18), qdd, np.zeros(3))
    tau = tau + arm * qdd
    E, r = _link_frames(model, root_quat, q)
    link, M, F = wrench
    E0 = E[0]
    fb = np.concatenate([E0.T @ M, E0.T @ F])
    tj = np.zeros(18)
    j = link
    links = model["links"]
    while j > 0:
        a = E[j] @ np.array(links[j]["axis"])
        tj[j - 1] = a @ (M - np.cross(r[j], F))
        j = links[j]["parent"]
    with_ext = max(np.abs(f0 - fb).max(), np.abs(tau - tj).max())
    without = max(np.abs(f0).max(), np.abs(tau).max())
    return with_ext, without


@pytest.mark.parametrize("kernel", KERNELS)
def test_known_answer_by_twin_envs(model, kernel, monkeypatch):
    """Pairs of equal envs at rest in free space, one of each pair pushed: every robot body (fixed ones included) and the ball, ENV and
    LOCAL space, at the centre of mass (force + torque) and at a point (force).  The velocity change of each pair, put into the RNEA with
    the applied wrench, leaves <= 2e-2 (fp32 state read back); without the external term the residual exceeds half the applied
    magnitude.  The ball: dv = F h / m, dw = h I^-1 (T + x F) times the kernel's angular damping."""
    nb = 22
    modes = [(space, at_pos) for space in ("env", "local") for at_pos in (False, True)]
    n = 2 * nb * len(modes)
    cfg = _free_cfg(n)
    sim = _sim(cfg, kernel, monkeypatch)
    sim.step(np.zeros((n, 18), np.float32))
    rng = np.random.default_rng(5)
    _inject_rest(sim, model, n, rng)
    rb = sim.rigid_body_states.reshape(n, nb, 13).astype(np.float64)
    rs0 = sim.root_states.reshape(n, 2, 13).astype(np.float64)
    ds0 = sim.dof_state.reshape(n, 18, 2).astype(np.float64)
    body_com = np.asarray(model["body_com"], float)
    F = np.zeros((n, nb, 3), np.float32); T = np.zeros((n, nb, 3), np.float32); X = np.zeros((n, nb, 3), np.float32)
    cases = []   # (env, body, space, at_pos, world force, world moment about the point, world point)
    k = 0
    for space, at_pos in modes:
        for b in range(nb):
            e = 2 * k + 1
            k += 1
            f = rng.normal(size=3); f *= rng.uniform(5.0, 20.0) / np.linalg.norm(f)
            t = rng.normal(size=3); t *= rng.uniform(5.0, 20.0) / np.linalg.norm(t) * 0.01   # N m on links of grams: keep the spin moderate
            pos, Rb = rb[e, b, 0:3], R.quat_to_mat(rb[e, b, 3:7])
            com_local = body_com[b] if b < nb - 1 else np.zeros(3)
            off = rng.uniform(-0.03, 0.03, 3)
            fw = Rb @ f if space == "local" else f
            if at_pos:
                t = np.zeros(3)
                if space == "local":
                    X[e, b] = com_local + off; xw = pos + Rb @ X[e, b]
                else:
                    xw = pos + Rb @ com_local + off; X[e, b] = xw
            else:
                xw = pos + Rb @ com_local
            tw = Rb @ t if space == "local" else t
            F[e, b] = f; T[e, b] = t
            cases.append((e, b, space, at_pos, fw, tw, xw))
    # one call per (space, at-position) group: the four groups touch disjoint envs
    for gi, (space, at_pos) in enumerate(modes):
        sel = np.zeros(n, bool)
        sel[[c[0] for c in cases if (c[2], c[3]) == (space, at_pos)]] = True
        Fg = np.where(sel[:, None, None], F, 0).astype(np.float32)
        Tg = np.where(sel[:, None, None], T, 0).astype(np.float32)
        ft, tt = torch.from_numpy(Fg).to(sim.dev).contiguous(), torch.from_numpy(Tg).to(sim.dev).contiguous()
        if at_pos:
            xt = torch.from_numpy(np.where(sel[:, None, None], X, 0).astype(np.float32)).to(sim.dev).contiguous()
            sim.sim.apply_body_forces(forces=ft, positions=xt, space=space)
        else:
            sim.sim.apply_body_forces(forces=ft, torques=tt, space=space)
    sim.simulate()
    rs1 = sim.root_states.reshape(n, 2, 13).astype(np.float64)
    ds1 = sim.dof_state.reshape(n, 18, 2).astype(np.float64)
    h = float(cfg.dt)
    damp = max(1.0 - h * float(cfg.ball_ang_damping), 0.0)
    mb, Ib = model["ball"]["mass"], model["ball"]["inertia"]
    worst, weakest = 0.0, np.inf
    for e, b, space, at_pos, fw, tw, xw in cases:
        mag = max(np.linalg.norm(fw), np.linalg.norm(tw))
        if b == nb - 1:   # the ball: a free body
            dv = (rs1[e, 1, 7:10] - rs1[e - 1, 1, 7:10])
            dw = (rs1[e, 1, 10:13] - rs1[e - 1, 1, 10:13])
            np.testing.assert_allclose(dv, fw * h / mb, rtol=1e-4, atol=1e-5, err_msg=str((kernel, space, at_pos)))
            mom = tw + np.cross(xw - rs0[e, 1, 0:3], fw)
            np.testing.assert_allclose(dw, h * mom / Ib * damp, rtol=1e-4, atol=1e-4, err_msg=str((kernel, space, at_pos)))
            assert np.abs(rs1[e, 0, 7:13] - rs1[e - 1, 0, 7:13]).max() < 1e-6   # the robot did not feel it
            continue
        assert np.abs(rs1[e, 1, 7:13] - rs1[e - 1, 1, 7:13]).max() < 1e-6     # the ball did not feel it
        qdd = (ds1[e, :, 1] - ds1[e - 1, :, 1]) / h
        a0 = np.concatenate([(rs1[e, 0, 10:13] - rs1[e - 1, 0, 10:13]) / h, (rs1[e, 0, 7:10] - rs1[e - 1, 0, 7:10]) / h])
        quat = rs0[e, 0, 3:7] / np.linalg.norm(rs0[e, 0, 3:7])
        link = model["body_link"][b]
        M = tw + np.cross(xw - rs0[e, 0, 0:3], fw)
        with_ext, without = _residuals(model, quat, ds0[e, :, 0], qdd, a0, float(cfg.armature), (link, M, fw))
        worst = max(worst, with_ext)
        weakest = min(weakest, without / mag)
        assert with_ext <= 2e-2, (kernel, b, space, at_pos, with_ext)
    assert weakest > 0.5, weakest
    # cleared after the launch: the next one moves nothing that was at rest
    sim.step(np.zeros((n, 18), np.float32))


def _state_of(sim):
    return np.concatenate([sim.root_states.ravel(), sim.dof_state.ravel()])


@pytest.mark.parametrize("kernel", KERNELS)
def test_forces_act_once_then_clear(model, kernel, monkeypatch):
    """S1: state X, apply, simulate -> Y1; X again, simulate without applying -> Y2.  S2 (never applies; a per-env parameter set to its
    default value so that it runs the same per-env-parameter kernel build the force-carrying kernels are made from): X, simulate -> Y3.
    Y2 == Y3 within 1e-5 (1 + |Y3|): the force-carrying instantiation with nothing pending evaluates the same expressions, but its extra
    (untaken) branches split basic blocks differently, so the compiler contracts a few different multiply-add pairs into FMAs -- last-bit
    differences (observed up to 1.1e-6 on MI355X; ws8q: a single element), not a different model.  Y1 != Y3."""
    n = 64
    cfg = abi.default_config(n, seed=11)
    s1, s2 = _sim(cfg, kernel, monkeypatch), _sim(abi.default_config(n, seed=11), kernel, monkeypatch)
    s2.set_env_params(abi.PARAM_FRICTION, np.full((n, 1), cfg.plane_friction, np.float32))
    for s in (s1, s2):
        s.step(np.zeros((n, 18), np.float32))
    rng = np.random.default_rng(2)
    rs, ds = s1.root_states, s1.dof_state
    f = torch.from_numpy(rng.uniform(-10, 10, (n, 22, 3)).astype(np.float32)).to(s1.dev).contiguous()

    def inject(s):
        s.set_root_states(rs); s.set_dof_state(ds)
    inject(s1); s1.sim.apply_body_forces(forces=f); s1.simulate(); y1 = _state_of(s1)
    inject(s1); s1.simulate(); y2 = _state_of(s1)
    inject(s2); s2.simulate(); y3 = _state_of(s2)
    np.testing.assert_allclose(y2, y3, rtol=1e-5, atol=1e-5)
    assert np.abs(y1 - y3).max() > 1e-3


@pytest.mark.parametrize("kernel", KERNELS)
def test_graph_replay_equals_eager(model, kernel, monkeypatch):
    """apply (from a static input tensor) + one env step captured in a torch.cuda.graph, replayed with two different force inputs: the
    same states / observations / rewards as the same calls made eagerly on a twin sim."""
    n = 64
    sg, se = _sim(abi.default_config(n, seed=4), kernel, monkeypatch), _sim(abi.default_config(n, seed=4), kernel, monkeypatch)
    dev = sg.dev
    act = torch.zeros((n, 18), dtype=torch.float32, device=dev)
    static_f = torch.zeros((n, 22, 3), dtype=torch.float32, device=dev)
    for s in (sg, se):
        s.sim.apply_body_forces(forces=static_f)   # first call: the pending buffer, the force-carrying kernels from here on
        s.sim.step(act.reshape(-1))
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        sg.sim.apply_body_forces(forces=static_f)
        sg.sim.step(act.reshape(-1))
    torch.cuda.synchronize()
    rng = np.random.default_rng(9)
    for _ in range(2):
        f = torch.from_numpy(rng.uniform(-15, 15, (n, 22, 3)).astype(np.float32)).to(dev)
        static_f.copy_(f)
        g.replay()
        se.sim.apply_body_forces(forces=f.contiguous())
        se.sim.step(act.reshape(-1))
        torch.cuda.synchronize()
        np.testing.assert_array_equal(_state_of(sg), _state_of(se))
        np.testing.assert_array_equal(sg.obs, se.obs)
        np.testing.assert_array_equal(sg.rew, se.rew)


@pytest.mark.parametrize("kernel", KERNELS)
def test_nonfinite_force_trips_only_its_env(model, kernel, monkeypatch):
    """A NaN force on one env: that env is reset by the non-finite guard and counted; every other env equals a twin run without it."""
    n = 64
    s1, s2 = _sim(abi.default_config(n, seed=6), kernel, monkeypatch), _sim(abi.default_config(n, seed=6), kernel, monkeypatch)
    for s in (s1, s2):
        s.step(np.zeros((n, 18), np.float32))
    f1 = np.zeros((n, 22, 3), np.float32); f1[:, 0, 0] = 3.0
    f2 = f1.copy(); f1[5, 7, 1] = np.nan
    s1.sim.apply_body_forces(forces=torch.from_numpy(f1).to(s1.dev))
    s2.sim.apply_body_forces(forces=torch.from_numpy(f2).to(s2.dev))
    for s in (s1, s2):
        s.step(np.zeros((n, 18), np.float32))
    c1 = s1.sim.nonfinite_counts.cpu().numpy(); c2 = s2.sim.nonfinite_counts.cpu().numpy()
    assert c1[5] == 1 and c1.sum() == 1 and c2.sum() == 0
    assert s1.reset_buf[5] == 1
    keep = np.arange(n) != 5
    a, b = s1.root_states.reshape(n, 2, 13), s2.root_states.reshape(n, 2, 13)
    np.testing.assert_array_equal(a[keep], b[keep])
    assert np.isfinite(a[5]).all()
    np.testing.assert_array_equal(s1.obs[keep], s2.obs[keep])


def _com(model, rb):
    links = model["links"]
    M = sum(L["mass"] for L in links)
    c = np.zeros((rb.shape[0], 3))
    for L in links:
        row = rb[:, L["body"]]
        Rl = np.stack([R.quat_to_mat(q) for q in row[:, 3:7]])
        c += L["mass"] * (row[:, 0:3] + np.einsum("nij,j->ni", Rl, np.asarray(L["com"])))
    return c / M


@pytest.mark.parametrize("kernel", KERNELS)
def test_push_moves_standing_robot(model, kernel, monkeypatch):
    """Default bez_kick (gravity, drives, ground): a 2-step horizontal push of 20 N on the torso of standing envs moves their centre of
    mass along the push relative to unpushed twins; NET_CONTACT_FORCE of the pushed step shows no trace of the push on the torso row."""
    n = 64
    sp, su = _sim(abi.default_config(n, seed=8), kernel, monkeypatch), _sim(abi.default_config(n, seed=8), kernel, monkeypatch)
    zero = np.zeros((n, 18), np.float32)
    push = np.zeros((n, 22, 3), np.float32); push[:, 0, 0] = 20.0
    for t in range(6):
        sp.sim.apply_body_forces(forces=torch.from_numpy(push if t < 2 else np.zeros_like(push)).to(sp.dev))
        su.sim.apply_body_forces(forces=torch.zeros((n, 22, 3), dtype=torch.float32, device=su.dev))
        sp.step(zero); su.step(zero)
    cp = _com(model, sp.rigid_body_states.reshape(n, 22, 13).astype(np.float64))
    cu = _com(model, su.rigid_body_states.reshape(n, 22, 13).astype(np.float64))
    ok = (sp.reset_buf == 0) & (su.reset_buf == 0)
    assert ok.sum() >= n // 2
    dx = (cp - cu)[ok]
    assert (dx[:, 0] > 1e-3).all(), dx[:, 0].min()
    assert np.abs(dx[:, 0]).mean() > 3 * np.abs(dx[:, 1]).mean()
