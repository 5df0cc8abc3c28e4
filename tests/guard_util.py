"""Helpers of the non-finite guard's GPU tests: a simulation per step kernel, a bit-exact snapshot of every buffer per env, fault
injection, and the twin run (A trips at step t; B is identical except that reset_buf[e] = 1 is set after its step t)."""
import numpy as np
import torch

from bez_isaacgym_amd import abi

STATE = (abi.TENSOR_ROOT_STATE, abi.TENSOR_DOF_STATE, abi.TENSOR_NET_CONTACT_FORCE, abi.TENSOR_DOF_TARGET, abi.TENSOR_PREV_LIN_VEL,
         abi.TENSOR_FEET, abi.TENSOR_GOAL)
LIVE = (abi.TENSOR_OBS, abi.TENSOR_REW, abi.TENSOR_RESET, abi.TENSOR_PROGRESS, abi.TENSOR_TIMEOUT)


def _sim(monkeypatch, n, kernel="ws8q", cleats=False, task=abi.TASK_KICK, guard=True, seed=11):
    from bez_isaacgym_amd.sim import BezSim
    monkeypatch.setenv("BEZ_SIM_KERNEL", kernel)   # read once, at bez_sim_create
    c = abi.default_config(n, seed=seed)
    c.task = task
    if cleats:
        c.flags |= abi.FLAG_CLEATS
    if not guard:
        c.flags &= ~abi.FLAG_NONFINITE_GUARD
    return BezSim(c, 0)


def _snap(sim):
    """Every buffer, per env: {tensor id: (N, k) array}; floats as their bit patterns (exact comparison, NaN included)."""
    n, out = sim.num_envs, {}
    for w in STATE + LIVE:
        t = (sim.refresh(w) if w in STATE else sim.tensor(w)).detach().clone().cpu().numpy()
        t = t.reshape(n, -1)
        out[w] = t.view(np.int32) if t.dtype == np.float32 else t
    return out


def _floats(a):
    return a.view(np.float32) if a.dtype == np.int32 else a


def _assert_others_equal(a, b, skip, where=""):
    keep = np.ones(next(iter(a.values())).shape[0], bool)
    keep[list(skip)] = False
    for w in a:
        np.testing.assert_array_equal(a[w][keep], b[w][keep], err_msg="tensor %d differs in an untouched env %s" % (w, where))


def _assert_env_finite(s, e):
    for w, v in s.items():
        if v.dtype == np.int32:
            assert np.isfinite(_floats(v[e])).all(), "tensor %d of the tripped env is not finite: %r" % (w, _floats(v[e]))


def _inject(sim, e, what, value):
    """value into env e's state: 'qd' = one joint velocity, 'q' = one joint position, 'root' = the torso's linear velocity z."""
    ids = torch.tensor([e * sim.num_actors], dtype=torch.int32, device=sim.device)
    if what in ("q", "qd"):
        dof = sim.refresh(abi.TENSOR_DOF_STATE).clone()
        dof[e * 18 + 7, 1 if what == "qd" else 0] = value
        sim.set_dof_state_tensor_indexed(dof.reshape(-1).contiguous(), ids)
    else:
        root = sim.refresh(abi.TENSOR_ROOT_STATE).clone()
        root[e * sim.num_actors, 9] = value
        sim.set_actor_root_state_tensor_indexed(root.reshape(-1).contiguous(), ids)


def _actions(rng, n):
    return torch.from_numpy(rng.uniform(-1, 1, (n, 18)).astype(np.float32)).cuda().reshape(-1).contiguous()


# ---- 2. the twin: A trips at step t; B is identical except that reset_buf[e] = 1 is set after its step t
def _twin(monkeypatch, n, e, kernel, cleats=False, task=abi.TASK_KICK, what="qd", value=float("nan"), dr=False):
    A, B = _sim(monkeypatch, n, kernel, cleats, task), _sim(monkeypatch, n, kernel, cleats, task)
    if dr:
        from bez_isaacgym_amd.utils.config import load_config
        params = load_config(["task=bez_kick"], resolve=True)["task"]["task"]["randomization_params"]
        for s in (A, B):
            s.set_randomization(abi.dr_config_from_params(params))
    rng = np.random.default_rng(5)
    for _ in range(4):
        act = _actions(rng, n)
        A.step(act); B.step(act)
    _inject(A, e, what, value)
    act = _actions(rng, n)
    A.step(act); B.step(act)
    torch.cuda.synchronize()
    sa, sb = _snap(A), _snap(B)
    _assert_env_finite(sa, e)
    assert _floats(sa[abi.TENSOR_REW])[e, 0] == 0.0 and sa[abi.TENSOR_RESET][e, 0] == 1
    assert sa[abi.TENSOR_PROGRESS][e, 0] == sb[abi.TENSOR_PROGRESS][e, 0] and sa[abi.TENSOR_TIMEOUT][e, 0] == sb[abi.TENSOR_TIMEOUT][e, 0]
    _assert_others_equal(sa, sb, [e], "at the trip")
    B.tensor(abi.TENSOR_RESET)[e] = 1
    for k in range(1, 21):
        act = _actions(rng, n)
        A.step(act); B.step(act)
        torch.cuda.synchronize()
        sa, sb = _snap(A), _snap(B)
        _assert_others_equal(sa, sb, [e], "at t + %d" % k)
        for w in sa:
            if w == abi.TENSOR_OBS and k == 1:   # the IMU columns may read prev_lin_vel (the replacement): finite is enough there
                np.testing.assert_array_equal(sa[w][e, :36], sb[w][e, :36])
                np.testing.assert_array_equal(sa[w][e, 39:], sb[w][e, 39:])
                assert np.isfinite(_floats(sa[w][e])).all()
            else:
                np.testing.assert_array_equal(sa[w][e], sb[w][e], err_msg="tensor %d of the tripped env at t + %d" % (w, k))
    cnt = A.nonfinite_counts.cpu().numpy()
    assert cnt[e] == 1 and cnt.sum() == 1 and B.nonfinite_counts.sum().item() == 0
    assert A.health() & abi.HEALTH_NONFINITE and B.health() == 0
