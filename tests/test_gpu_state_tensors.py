"""GPU: the state-tensor boundary of bez_sim.hip -- what rl_games and the task code see -- against references that leave no room for
an outlier budget.

  * refresh_rigid_body_kernel<CL> (FK + mat_to_quat): the state set of tests/state_sets.py (random SO(3) roots with both
    signs, mat_to_quat's branch seams, joints over their range and at their limits, fast joints and roots, |x|, |y| to 100 m) on the
    default, cleats and box assets x the kick (ball row) and walk / orient (no ball) layouts, at sizes around the 64-thread blocks;
    against the fp64 FD reference (default asset) and the fp64 oracle (every asset).  Bar per field: 3x the fp32 oracle's worst error
    on the same states + 2 fp32 ulps of the value.
  * refresh / scatter / indexed setters, bit for bit against a numpy model of Isaac Gym's contract: empty, single, unsorted, strided,
    all-actor, ball-actor and invalid id sets; after every call every refreshable tensor is snapshot and only the intended rows may
    change.
  * reset_indexed against Oracle.reset_idx, bit for bit (partial, unsorted, overlapping, with invalid ids for the HIP side only).
  * get_env_params / set_env_params: the default rows, set -> get, set None -> the defaults again (the packed per-joint copy included);
    the default rows also from a side stream with one synchronisation at the end (the call only enqueues work).
  * every BezTensor id: the header's dtype and shape per task and asset, a refresh that succeeds and returns the same memory.
  * create / destroy over the lazily allocated buffers leaves the free device memory where it was.
"""
import numpy as np
import pytest
import torch

from bez_isaacgym_amd import abi
from tests.state_sets import DOF_LOWER, DOF_UPPER, FIELDS, NB, align_quat, ball_states, fd_reference, field_errors, generate_states, oracle_rows, ulp32
from tests.gpu_util import ASSETS, _bars, _dev, _host, _ids, _sim, _write_states
from tests.sim_cfg import make_cfg

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 65, 300)
NMAX = max(SIZES)


@pytest.fixture(scope="module")
def gen():
    root, dof, cases = generate_states(NMAX)
    ball = ball_states(NMAX)
    return dict(root=root, dof=dof, ball=ball, cases=cases, fd=fd_reference(root, dof))


def _check(rows, ref, bars, what):
    err = field_errors(rows, ref)
    worst = {}
    for name, sl in FIELDS:
        b = bars[name][: rows.shape[0]]
        bad = err[name] > b
        assert not bad.any(), (what, name, float(err[name].max()), [tuple(x) for x in np.argwhere(bad)[:5]])
        worst[name] = (float(err[name].max()), float(np.max(b)))
    return worst


@pytest.mark.parametrize("task", ["bez_kick", "bez_walk", "bez_orient"])
@pytest.mark.parametrize("asset", list(ASSETS))
def test_rigid_body_refresh_against_fp64_references(gen, asset, task):
    """every body row of every env: position, quaternion (sign-aligned, unit to 1e-6), origin velocity and angular velocity against the
    fp64 oracle (and on the default asset the FD reference); the IMU row (body 1) rides on the root; the ball row is the root tensor's"""
    kw = ASSETS[asset]
    cfg = lambda n: make_cfg(n, task=task, seed=5, **kw)
    root, dof, ball = gen["root"], gen["dof"], gen["ball"]
    o64 = oracle_rows(cfg(NMAX), "f64", root, dof, ball)
    o32 = oracle_rows(cfg(NMAX), "f32", root, dof, ball)
    nb = o64.shape[1] - (1 if task == "bez_kick" else 0)
    assert nb == (29 if asset == "cleats" else 21)
    bars_o = _bars(field_errors(o32[:, :nb], o64[:, :nb].astype(np.float64)), o64[:, :nb].astype(np.float64))
    if asset == "default":
        fd = gen["fd"]
        bars_fd = _bars(field_errors(o32[:, :NB], fd), fd)
    report = {}
    for n in SIZES:
        sim = _sim(cfg(n))
        rs = _write_states(sim, root[:n], dof[:n], ball[:n])
        rb = _host(sim.refresh(abi.TENSOR_RIGID_BODY_STATE)).reshape(n, -1, 13)
        rt = _host(sim.refresh(abi.TENSOR_ROOT_STATE)).reshape(n, sim.num_actors, 13)
        assert rb.shape[1] == o64.shape[1] == sim.num_bodies
        np.testing.assert_array_equal(rt, rs)
        assert np.isfinite(rb).all()
        qn = np.linalg.norm(rb[:, :nb, 3:7].astype(np.float64), axis=-1)
        assert np.abs(qn - 1).max() <= 1e-6, float(np.abs(qn - 1).max())
        report["oracle", n] = _check(rb[:, :nb], o64[:n, :nb].astype(np.float64), bars_o, (asset, task, n, "fp64 oracle"))
        if asset == "default":
            report["fd", n] = _check(rb[:, :NB], fd[:n], bars_fd, (asset, task, n, "FD reference"))
        # the IMU link (body 1) is the torso origin: the same row as body 0, bit for bit; position and velocities are the root's
        # bits; its quaternion went through quat_to_mat -> mat_to_quat
        np.testing.assert_array_equal(rb[:, 1].view(np.uint32), rb[:, 0].view(np.uint32))
        np.testing.assert_array_equal(rb[:, 1, 0:3].view(np.uint32), rt[:, 0, 0:3].view(np.uint32))
        np.testing.assert_array_equal(rb[:, 1, 7:13].view(np.uint32), rt[:, 0, 7:13].view(np.uint32))
        np.testing.assert_allclose(align_quat(rb[:, 1, 3:7], rt[:, 0, 3:7]), rt[:, 0, 3:7], rtol=0, atol=3e-7)
        if task == "bez_kick":
            np.testing.assert_array_equal(rb[:, nb].view(np.uint32), rt[:, 1].view(np.uint32))
            np.testing.assert_array_equal(rb[:, nb], ball[:n])
        sim.close()
    print("worst error / bar:", {k: v for k, v in report.items() if k[1] == NMAX})


# ---------------------------------------------------------------- the tensor table: every id, its documented dtype and shape

def _documented_tensors(n, nact, nbe, nobs):
    """dtype and shape of every BezTensor as include/bez_sim.h documents them beside the enum (A actors, B bodies, OBS width)"""
    f32, i64 = torch.float32, torch.int64
    return {abi.TENSOR_ROOT_STATE: (f32, (n * nact, 13)), abi.TENSOR_DOF_STATE: (f32, (n * 18, 2)),
            abi.TENSOR_RIGID_BODY_STATE: (f32, (n * nbe, 13)), abi.TENSOR_NET_CONTACT_FORCE: (f32, (n * nbe, 3)),
            abi.TENSOR_OBS: (f32, (n, nobs)), abi.TENSOR_REW: (f32, (n,)), abi.TENSOR_RESET: (i64, (n,)),
            abi.TENSOR_PROGRESS: (i64, (n,)), abi.TENSOR_TIMEOUT: (i64, (n,)), abi.TENSOR_DOF_TARGET: (f32, (n, 18)),
            abi.TENSOR_PREV_LIN_VEL: (f32, (n, 3)), abi.TENSOR_FEET: (f32, (n, 8)), abi.TENSOR_GOAL: (f32, (n, 2)),
            abi.TENSOR_RANDOMIZE_BUF: (i64, (n,)), abi.TENSOR_DR_NOISE: (f32, (4,)), abi.TENSOR_NONFINITE_COUNT: (i64, (n,)),
            abi.TENSOR_HEALTH: (i64, (1,))}


@pytest.mark.parametrize("task", ["bez_kick", "bez_walk", "bez_orient"])
@pytest.mark.parametrize("asset", ["default", "cleats"])
def test_every_tensor_id_has_its_documented_layout_and_refreshes(asset, task):
    """tensor(id) for every id below TENSOR_COUNT: the header's dtype and shape for this task and asset; refresh(id) succeeds -- a no-op
    for the always-live ones, TENSOR_RANDOMIZE_BUF and TENSOR_DR_NOISE included -- and hands back a view of the same memory; the
    first id past the table is an error for both"""
    from bez_isaacgym_amd.sim import BezSimError
    n = 3
    sim = _sim(make_cfg(n, task=task, seed=2, **ASSETS[asset]))
    kick = task == "bez_kick"
    nact, nbe, nobs = (2 if kick else 1), (29 if asset == "cleats" else 21) + (1 if kick else 0), (54 if kick else 52)
    assert (sim.num_actors, sim.num_bodies, sim.num_obs) == (nact, nbe, nobs)
    doc = _documented_tensors(n, nact, nbe, nobs)
    assert sorted(doc) == list(range(abi.TENSOR_COUNT))
    for which in range(abi.TENSOR_COUNT):
        t = sim.tensor(which)
        assert (t.dtype, tuple(t.shape)) == doc[which] and t.is_contiguous() and t.data_ptr() != 0, which
        r = sim.refresh(which)
        assert r.data_ptr() == t.data_ptr() and (r.dtype, tuple(r.shape)) == doc[which], which
    torch.cuda.synchronize()
    for call in (sim.tensor, sim.refresh):
        with pytest.raises(BezSimError):
            call(abi.TENSOR_COUNT)
    sim.close()


# ---------------------------------------------------------------- setters: bit for bit against a numpy model of the contract

_REFRESH = {"root": abi.TENSOR_ROOT_STATE, "dof": abi.TENSOR_DOF_STATE, "contact": abi.TENSOR_NET_CONTACT_FORCE,
            "targets": abi.TENSOR_DOF_TARGET, "prev": abi.TENSOR_PREV_LIN_VEL, "feet": abi.TENSOR_FEET, "goal": abi.TENSOR_GOAL}
_LIVE = {"obs": abi.TENSOR_OBS, "rew": abi.TENSOR_REW, "reset": abi.TENSOR_RESET, "progress": abi.TENSOR_PROGRESS,
         "timeout": abi.TENSOR_TIMEOUT}


def _snapshot(sim):
    out = {k: _host(sim.refresh(w)) for k, w in _REFRESH.items()}
    out.update({k: _host(sim.tensor(w)) for k, w in _LIVE.items()})
    out["rigid"] = _host(sim.refresh(abi.TENSOR_RIGID_BODY_STATE)).reshape(sim.num_envs, sim.num_bodies, 13)
    return out


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _assert_model(sim, model, touched, what):
    """every refreshable / live tensor equals the model bit for bit; the rigid-body rows of envs whose root or DOF state was not
    written are unchanged bit for bit (the kick layout's ball row: the root tensor's ball row)"""
    snap = _snapshot(sim)
    for k in list(_REFRESH) + list(_LIVE):
        np.testing.assert_array_equal(_bits(snap[k]), _bits(model[k]), err_msg="%s: %s" % (what, k))
    keep = np.ones(sim.num_envs, bool)
    keep[list(touched)] = False
    np.testing.assert_array_equal(_bits(snap["rigid"][keep]), _bits(model["rigid"][keep]), err_msg="%s: untouched rigid-body rows" % what)
    if sim.num_actors == 2:
        np.testing.assert_array_equal(_bits(snap["rigid"][:, -1]), _bits(snap["root"].reshape(-1, 2, 13)[:, 1]), err_msg=what)
    model["rigid"] = snap["rigid"]


def _values(rng, shape):
    """fp32 values with the bit patterns a lossy path would change: -0.0, subnormals, large magnitudes"""
    v = rng.normal(size=shape).astype(np.float32)
    flat = v.reshape(-1)
    k = rng.integers(0, flat.size, max(1, flat.size // 50))
    flat[k[0::3]] = np.float32(-0.0)
    flat[k[1::3]] = np.float32(3e-39) * rng.choice([-1, 1], len(k[1::3])).astype(np.float32)
    flat[k[2::3]] = np.float32(1e30) * rng.normal(size=len(k[2::3])).astype(np.float32)
    return v


def _id_sets(n, nact, rng):
    A = n * nact
    sets = [("empty", np.zeros(0, np.int64)), ("single_first", np.array([0])), ("single_last", np.array([A - 1]))]
    # counts whose count*13 / count*36 / count*18 cross a 256-thread block edge (19/20, 7/8, 14/15), and a larger one
    for c in (7, 8, 14, 15, 19, 20, 197):
        if c <= A:
            sets.append(("unsorted_%d" % c, rng.permutation(A)[:c]))
    sets.append(("strided", np.arange(1, A, 3)[::-1]))
    sets.append(("all_actors", rng.permutation(A)))
    if nact == 2:
        sets.append(("ball_actors", rng.permutation(np.arange(1, A, 2))))
    bad = np.array([-1, A, np.iinfo(np.int32).min, np.iinfo(np.int32).max])
    sets.append(("invalid_only", bad))
    sets.append(("mixed_invalid", rng.permutation(np.concatenate([rng.permutation(A)[: min(A, 9)], bad]))))
    return sets


@pytest.mark.parametrize("nact", [1, 2])
@pytest.mark.parametrize("n", [1, 257, 4097])
def test_setters_and_refreshes_bit_exact(n, nact):
    """set_*_tensor round trips, then each indexed setter (root, DOF, target) with every id set: only the listed valid actors change,
    with the source's bits; the DOF and target setters ignore ball actors; ids -1, n*nact, INT32_MIN / MAX are ignored."""
    rng = np.random.default_rng(n * 10 + nact)
    sim = _sim(make_cfg(n, task="bez_kick" if nact == 2 else "bez_walk", seed=9))
    assert sim.num_actors == nact
    nbe = sim.num_bodies
    model = _snapshot(sim)
    for name, setter, key, shape in (("targets", sim.set_dof_position_target_tensor, "targets", (n, 18)),
                                     ("contact", sim.set_net_contact_force_tensor, "contact", (n * nbe, 3)),
                                     ("prev", sim.set_prev_lin_vel_tensor, "prev", (n, 3)),
                                     ("goal", sim.set_goal_tensor, "goal", (n, 2))):
        v = _values(rng, shape)
        setter(_dev(v))
        model[key] = v
        _assert_model(sim, model, (), "set_%s_tensor" % name)
    A = n * nact
    for label, ids in _id_sets(n, nact, rng):
        valid = ids[(ids >= 0) & (ids < A)]
        robots = valid[valid % nact == 0]
        # root states: every valid actor row, robot or ball
        src = _values(rng, (A, 13))
        sim.set_actor_root_state_tensor_indexed(_dev(src), _ids(ids))
        model["root"][valid] = src[valid]
        _assert_model(sim, model, set((valid // nact).tolist()), "root_indexed " + label)
        # DOF states: robot actors only
        src = _values(rng, (n, 18, 2))
        sim.set_dof_state_tensor_indexed(_dev(src), _ids(ids))
        d = model["dof"].reshape(n, 18, 2)
        d[robots // nact] = src[robots // nact]
        _assert_model(sim, model, set((robots // nact).tolist()), "dof_indexed " + label)
        # position targets: robot actors only
        src = _values(rng, (n, 18))
        sim.set_dof_position_target_tensor_indexed(_dev(src), _ids(ids))
        model["targets"][robots // nact] = src[robots // nact]
        _assert_model(sim, model, (), "target_indexed " + label)
    sim.close()


# ---------------------------------------------------------------- reset_indexed against the oracle

def _scramble(o, g, rng, gen):
    """the same fp32 state, far from any reset state, into both"""
    n, nact = o.n, o.nact
    rs = np.zeros((n, nact, 13), np.float32)
    rs[:, 0] = gen["root"][:n]
    if nact == 2:
        rs[:, 1] = gen["ball"][:n]
    state = dict(root_states=rs.reshape(-1, 13), dof_state=gen["dof"][:n].reshape(-1, 2),
                 targets=rng.uniform(-1, 1, (n, 18)).astype(np.float32),
                 contact_forces=rng.normal(0, 10, (n * o.nbe, 3)).astype(np.float32),
                 prev_lin_vel=rng.normal(size=(n, 3)).astype(np.float32),
                 goal=rng.uniform(-3, 3, (n, 2)).astype(np.float32))
    for k, v in state.items():
        getattr(o, "set_" + k)(v); getattr(g, "set_" + k)(v)
    prog = rng.integers(0, 500, n).astype(np.int64)
    for x in (o, g):
        x.set_progress(prog); x.set_reset(np.ones(n, np.int64))
    return state


def _compare_to_oracle(o, g, what):
    for k in ("dof_state", "root_states", "targets", "progress_buf", "reset_buf", "timeout_buf", "goal", "contact_forces",
              "prev_lin_vel", "feet"):
        np.testing.assert_array_equal(_bits(getattr(g, k)), _bits(getattr(o, k)), err_msg="%s: %s" % (what, k))


@pytest.mark.parametrize("task", ["bez_kick", "bez_walk", "bez_orient"])
def test_reset_indexed_matches_oracle_bit_for_bit(gen, task):
    """partial unsorted, then overlapping resets with env_id_offset != 0: DOF and root state (both actors), targets, progress, the
    reset buffer, the goal (one draw per call for walk / orient), and the contact rows (zeroed for the reset envs only).  Invalid ids
    go to the HIP side only; an empty call changes nothing and draws no goal; a call with only invalid ids draws one, like the
    oracle's empty call.  The second, overlapping reset matches only if the episode counters moved for the listed envs alone."""
    from oracle.bez_oracle import Oracle
    from tests.sim_adapter import SimAdapter
    n = 300
    cfg = lambda: make_cfg(n, task=task, seed=1234, env_id_offset=1000)
    o, g = Oracle(cfg()), SimAdapter(cfg())
    _compare_to_oracle(o, g, "after creation")
    rng = np.random.default_rng(21)
    state = _scramble(o, g, rng, gen)
    _compare_to_oracle(o, g, "scrambled")
    bad = np.array([-1, n, -7, np.iinfo(np.int32).max])
    first = rng.permutation(n)[:97]
    second = rng.permutation(np.concatenate([first[:40], rng.permutation(np.setdiff1d(np.arange(n), first))[:80]]))
    reset_once = np.zeros(n, bool)
    after_first = None
    for label, ids in (("first", first), ("empty", np.zeros(0, np.int64)), ("invalid_only", bad), ("second", second)):
        g.reset_idx(rng.permutation(np.concatenate([ids, bad])) if label in ("first", "second") else ids)
        listed = ids[(ids >= 0) & (ids < n)]
        if label != "empty":
            o.reset_idx(listed)
        _compare_to_oracle(o, g, "reset " + label)
        reset_once[listed] = True
        cf = g.contact_forces.reshape(n, o.nbe, 3)
        assert (cf[reset_once] == 0).all()
        np.testing.assert_array_equal(cf[~reset_once], state["contact_forces"].reshape(n, o.nbe, 3)[~reset_once])
        if task != "bez_kick" and len(listed):   # one goal per call, shared by every env it resets
            goal = g.goal
            assert (goal[listed] == goal[listed[0]]).all()
        if label == "first":
            after_first = g.dof_state.reshape(n, 18, 2).copy()
    # the 40 envs reset twice took a fresh draw the second time (their episode counter moved), the envs reset once kept theirs
    twice = np.intersect1d(first, second)
    assert len(twice) == 40
    d = g.dof_state.reshape(n, 18, 2)
    assert (d[twice, :, 1] != after_first[twice, :, 1]).any(axis=1).all()
    once = np.setdiff1d(first, second)
    np.testing.assert_array_equal(d[once], after_first[once])


# ---------------------------------------------------------------- env params

def _default_rows(cfg, n):
    f = np.float32
    return {abi.PARAM_FRICTION: np.full((n, 1), cfg.plane_friction, f), abi.PARAM_KP_SCALE: np.ones((n, 18), f),
            abi.PARAM_KD_SCALE: np.ones((n, 18), f), abi.PARAM_MASS_SCALE: np.ones((n, 19), f),
            abi.PARAM_GRAVITY: np.tile(np.array(cfg.gravity[:], f), (n, 1)),
            abi.PARAM_DOF_LOWER: np.tile(DOF_LOWER.astype(f), (n, 1)), abi.PARAM_DOF_UPPER: np.tile(DOF_UPPER.astype(f), (n, 1))}


@pytest.mark.parametrize("n", [1, 257])
def test_env_params_defaults_round_trip_and_unset(n):
    """for every PARAM_*: before any set, get returns the default rows (the config's friction and gravity, unit scales, the URDF's
    joint limits in fp32 -- the oracle's too); set -> get is bit-exact; set None -> the default rows again; and the default rows of all
    seven read back to back on a side stream, with nothing but one device synchronisation at the end"""
    from oracle.bez_oracle import Oracle
    cfg = make_cfg(n, seed=4)
    sim, o = _sim(cfg), Oracle(make_cfg(n, seed=4))
    dflt = _default_rows(cfg, n)
    rng = np.random.default_rng(n)
    for p in range(abi.PARAM_COUNT):
        w = abi.PARAM_WIDTH[p]
        got = _host(sim.get_env_params(p))
        assert got.shape == (n, w)
        np.testing.assert_array_equal(_bits(got), _bits(dflt[p]), err_msg="default rows of param %d" % p)
        np.testing.assert_array_equal(_bits(got), _bits(o.get_env_params(p)), err_msg="oracle's default rows of param %d" % p)
        for _ in range(2):   # the second set reuses the allocation
            v = _values(rng, (n, w))
            sim.set_env_params(p, _dev(v))
            np.testing.assert_array_equal(_bits(_host(sim.get_env_params(p))), _bits(v), err_msg="set -> get of param %d" % p)
        sim.set_env_params(p, None)
        np.testing.assert_array_equal(_bits(_host(sim.get_env_params(p))), _bits(dflt[p]), err_msg="set None of param %d" % p)
    # the default rows only enqueue work: all seven on a side stream with no synchronisation in between, then one for the device
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        got = [sim.get_env_params(p) for p in range(abi.PARAM_COUNT)]
    torch.cuda.synchronize()
    for p in range(abi.PARAM_COUNT):
        np.testing.assert_array_equal(_bits(got[p].cpu().numpy()), _bits(dflt[p]), err_msg="side-stream default rows of param %d" % p)
    sim.close()


def test_destroy_returns_every_buffer():
    """every lazily allocated buffer has the sim as its owner: after one create / destroy per flag combination -- the actuator record,
    the extra ground points set through set_flags, a randomisation set then unset, the external-wrench buffer -- the free device
    memory is back at its starting value within the allocator's granularity, which is what a plain create / destroy pair moves it by.
    (A first, unmeasured pass loads the code objects of the kernel variants these sims launch and fills torch's own pool.)"""
    from bez_isaacgym_amd.utils.config import load_config
    n = 65
    dr = abi.dr_config_from_params(load_config(["task=bez_kick"], resolve=True)["task"]["task"]["randomization_params"])
    act, forces = torch.zeros(n * 18, device="cuda:0"), torch.ones(n * 22, 3, device="cuda:0")

    def free():
        torch.cuda.synchronize()
        return torch.cuda.mem_get_info(0)[0]

    def create_use_destroy(flags, use):
        cfg = make_cfg(n, seed=1)
        cfg.flags |= flags
        sim = _sim(cfg)
        use(sim)
        sim.step(act)
        torch.cuda.synchronize()
        sim.close()

    def randomise_and_unset(sim):
        sim.set_randomization(dr)
        sim.step(act)
        sim.set_randomization(None)
        for p in range(abi.PARAM_COUNT):
            sim.set_env_params(p, None)

    def every_combination():
        create_use_destroy(abi.FLAG_DOF_FORCE, lambda sim: (sim.step(act), sim.refresh_actuator_tensors()))
        create_use_destroy(0, lambda sim: sim.set_flags(int(sim.cfg.flags) | abi.FLAG_ALL_GROUND_SHAPES))
        create_use_destroy(0, randomise_and_unset)
        create_use_destroy(0, lambda sim: sim.apply_body_forces(forces=forces))

    every_combination()
    start = free()
    _sim(make_cfg(n, seed=1)).close()
    granularity = abs(free() - start)
    every_combination()
    end = free()
    print("free device memory: %d before, %d after, granularity %d" % (start, end, granularity))
    assert abs(end - start) <= granularity, (start, end, granularity)


def _step_outputs(sim, act):
    sim.step(_dev(act))
    return [_host(sim.tensor(abi.TENSOR_OBS)), _host(sim.refresh(abi.TENSOR_ROOT_STATE)), _host(sim.refresh(abi.TENSOR_DOF_STATE)),
            _host(sim.tensor(abi.TENSOR_REW))]


def test_env_params_unset_restores_the_packed_params():
    """the step reads KP / KD scales and joint limits from one packed per-joint copy: after set None of some of them, a step must be
    bit-identical to a sim that only ever set the others, and after set None of all of them, to a sim that never set any"""
    n = 257
    rng = np.random.default_rng(3)
    kp, kd = rng.uniform(0.5, 1.5, (n, 18)).astype(np.float32), rng.uniform(0.5, 1.5, (n, 18)).astype(np.float32)
    lo = (DOF_LOWER[None] + rng.uniform(-0.2, 0.2, (n, 18))).astype(np.float32)
    hi = (DOF_UPPER[None] + rng.uniform(-0.2, 0.2, (n, 18))).astype(np.float32)
    act = rng.uniform(-1, 1, (n, 18)).astype(np.float32)
    packed = {abi.PARAM_KP_SCALE: kp, abi.PARAM_KD_SCALE: kd, abi.PARAM_DOF_LOWER: lo, abi.PARAM_DOF_UPPER: hi}
    cfg = lambda: make_cfg(n, seed=6)
    a, b = _sim(cfg()), _sim(cfg())
    for p, v in packed.items():
        a.set_env_params(p, _dev(v))
    a.set_env_params(abi.PARAM_KP_SCALE, None); a.set_env_params(abi.PARAM_DOF_LOWER, None)
    b.set_env_params(abi.PARAM_KD_SCALE, _dev(kd)); b.set_env_params(abi.PARAM_DOF_UPPER, _dev(hi))
    for x, y in zip(_step_outputs(a, act), _step_outputs(b, act)):
        np.testing.assert_array_equal(_bits(x), _bits(y))
    c, d = _sim(cfg()), _sim(cfg())
    for p, v in packed.items():
        c.set_env_params(p, _dev(v))
    for p in packed:
        c.set_env_params(p, None)
    for x, y in zip(_step_outputs(c, act), _step_outputs(d, act)):
        np.testing.assert_array_equal(_bits(x), _bits(y))
    # and the scales do reach the step (the comparison above is not vacuous)
    e = _sim(cfg())
    e.set_env_params(abi.PARAM_KP_SCALE, _dev(kp))
    assert not np.array_equal(_step_outputs(e, act)[0], _step_outputs(_sim(cfg()), act)[0])
    for s in (a, b, c, d, e):
        s.close()
