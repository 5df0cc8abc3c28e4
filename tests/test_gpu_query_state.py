"""GPU: query states (include/bez_sim.h "Query states") -- the dynamics queries on states the caller supplies.

  twin         a query state of M rows filled with set() answers every query, and refreshes its three tensors, to the bit as a sim of
               num_envs = M holding the same state does: same kernels, same input bits.  M crosses the 16-row tiles and limb_ik's 32-row
               tile, below and above the parent's N, both assets, with and without a ball.
  gather       env_ids hands row i the parameter rows of env env_ids[i] (repeats, ids outside 0 .. N-1: the default rows), to the bit as
               a twin given those rows; a parameter the parent never allocated stays the default.
  capture      rows taken from a stepped, randomised parent answer as the live queries do for those envs; a row with an id outside
               0 .. N-1 keeps what set() gave it.
  untouched    a sim whose query state is set, captured, asked and refreshed between its steps stays bitwise the sim that has none.
  known answer the rigid-body rows of a query state against the fp64 finite-difference reference (a twin could be wrong the same way).
  refusals     rc -1 with a message; device memory returns after close(); a sim without query states allocates nothing new.
"""
import ctypes as C
import gc

import numpy as np
import pytest
import torch

from bez_isaacgym_amd import abi
from tests.gpu_util import _bars, _bits, _dev, _dr_cfg, _free, _host, _ids, _sim, _write_states
from tests.sim_cfg import make_cfg
from tests.state_sets import NB, ball_states, fd_reference, field_errors, generate_states, oracle_rows

pytestmark = pytest.mark.gpu

NMAX = 64
OFFSETS = [[0.01 * c, -0.02, 0.03 * c] for c in range(5)]
WEIGHTS = [[1.0, 1.0], [1.0, 0.0], [1.0, 0.5], [0.0, 1.0], [2.0, 1.0]]


@pytest.fixture(scope="module")
def gen():
    """NMAX seeded rows of everything a query takes: states, udot, force, body wrenches and points, IK targets; computed once, left unchanged"""
    root, dof, _ = generate_states(NMAX)
    rng = np.random.default_rng(71)
    quat = rng.normal(size=(NMAX, 5, 4))
    targets = np.concatenate([rng.uniform(-0.3, 0.3, (NMAX, 5, 3)), quat / np.linalg.norm(quat, axis=2, keepdims=True)], axis=2)
    f32 = lambda a: a.astype(np.float32)
    return dict(root=root, dof=dof, ball=ball_states(NMAX), udot=f32(rng.uniform(-10, 10, (NMAX, 24))), force=f32(rng.uniform(-5, 5, (NMAX, 24))),
                F=f32(rng.uniform(-20, 20, (NMAX, 30, 3))), T=f32(rng.uniform(-2, 2, (NMAX, 30, 3))), X=f32(rng.uniform(-0.1, 0.1, (NMAX, 30, 3))),
                targets=f32(targets))


def rows_of(gen, rows):
    """the inputs of the given rows (a count, or an index array)"""
    pick = np.arange(rows) if isinstance(rows, int) else np.asarray(rows)
    return {k: v[pick] for k, v in gen.items()}


def ask(obj, inp, tensors=True):
    """{label: host array with the rows first} of every query call on `obj`, a BezSim or a QueryState -- they share the methods -- holding
    len(inp["root"]) rows: both base modes, udot / force given and None, the `want` subsets and term sets the GPU tests of each call
    exercise, limb_ik with 0 and 3 iterations -- and, `tensors`, the refreshed rigid-body rows, Jacobian and mass matrix"""
    m, nbe = obj.num_envs, obj.num_bodies
    dev = lambda a: _dev(a).view(a.shape)
    udot, force, targets = dev(inp["udot"]), dev(inp["force"]), dev(inp["targets"])
    F, T, X = (dev(np.ascontiguousarray(inp[k][:, :nbe])) for k in "FTX")
    out = {}

    def put(label, *ts):
        for k, t in enumerate(ts):
            if t is not None:
                out["%s#%d" % (label, k)] = _host(t).reshape(m, -1)

    for u, terms in ((None, abi.ID_ALL), (udot, abi.ID_ALL), (udot, abi.ID_INERTIA), (None, abi.ID_VELOCITY | abi.ID_GRAVITY), (None, abi.ID_GRAVITY),
                     (udot, abi.ID_INERTIA | abi.ID_VELOCITY)):
        put("id %s %d" % (u is not None, terms), obj.inverse_dynamics(u, terms))
    for f, bias, fixed in ((None, 6, False), (force, 6, False), (force, 0, False), (force, 2, False), (None, 4, True), (force, 6, True), (force, 0, True)):
        put("fd %s %d %s" % (f is not None, bias, fixed), obj.forward_dynamics(f, bias, fixed))
    for offsets, fixed, want in ((None, False, ("jac", "jminv", "w", "lambda")), (OFFSETS, False, ("jac", "jminv", "w", "lambda")), (None, False, ("jac",)),
                                 (OFFSETS, False, ("jminv",)), (None, False, ("w",)), (OFFSETS, False, ("lambda",)), (None, False, ("jminv", "lambda")),
                                 (OFFSETS, True, ("jac", "jminv", "w")), (None, True, ("w",))):
        put("os %s %s %s" % (offsets is not None, fixed, "+".join(want)), *obj.operational_space(offsets, fixed, want=want))
    put("cm state", *obj.centroidal())
    put("cm matrix", *obj.centroidal(want_matrix=True))
    for u, terms, space in ((None, abi.ACC_MOTION, "env"), (udot, abi.ACC_MOTION, "env"), (udot, abi.ACC_ALL, "local"), (udot, abi.ACC_UDOT, "env"),
                            (None, abi.ACC_VELOCITY, "local"), (None, abi.ACC_GRAVITY, "env")):
        put("acc %s %d %s" % (u is not None, terms, space), obj.body_accelerations(u, terms, space))
    for kw in (dict(forces=F, torques=T, positions=X), dict(forces=F), dict(torques=T, space="local", at="origin"), dict(forces=F, torques=T, space="local"),
               dict(forces=F, positions=X, space="local"), dict(forces=F, torques=T, at="origin")):
        put("gf " + " ".join(sorted(kw)) + str(kw.get("space")) + str(kw.get("at")), obj.generalized_forces(**kw))
    for iters, space, kw in ((0, "env", {}), (0, "root", {}), (3, "env", {}), (3, "root", dict(offsets=OFFSETS, max_step=0.2))):
        put("ik %d %s %d" % (iters, space, len(kw)), *obj.limb_ik(targets, WEIGHTS, iters=iters, space=space, **kw))
    for want in (("ground", "ball", "pairs"), ("ground",), ("ball",), ("pairs",), ("ground", "pairs")):
        put("px " + "+".join(want), *obj.proximity(want=want))
    if tensors:
        J, M = obj.dynamics_tensor("jacobian"), obj.dynamics_tensor("mass_matrix")
        obj.refresh_dynamics_tensors("jacobian")
        put("jacobian alone", J)
        obj.refresh_dynamics_tensors()
        put("tensors", obj.refresh(abi.TENSOR_RIGID_BODY_STATE), J, M)
    return out


def same_bits(a, b, rows_a=None, rows_b=None, what=""):
    assert sorted(a) == sorted(b) and a
    for k in a:
        x, y = a[k] if rows_a is None else a[k][rows_a], b[k] if rows_b is None else b[k][rows_b]
        assert x.shape == y.shape and x.size, (what, k)
        bad = np.flatnonzero((_bits(x) != _bits(y)).any(axis=1))
        assert bad.size == 0, "%s %s: rows %s differ" % (what, k, bad[:8])


def fill(qs, inp, env_ids=None):
    ball = _dev(inp["ball"]).view(-1, 13) if qs.has_ball else None
    qs.set(_dev(inp["root"]).view(-1, 13), _dev(inp["dof"]).view(-1, 18, 2), ball, None if env_ids is None else _ids(env_ids))


def twin_of(cfg_of, inp, params=None):
    """a sim of as many envs as `inp` has rows, holding those states (and the given parameter rows)"""
    m = len(inp["root"])
    sim = _sim(cfg_of(m))
    _write_states(sim, inp["root"], inp["dof"], inp["ball"])
    for p, rows in (params or {}).items():
        sim.set_env_params(p, _dev(rows))
    return sim


# ---------------------------------------------------------------- 1. twin, to the bit

@pytest.mark.parametrize("task", ["bez_kick", "bez_walk"])
@pytest.mark.parametrize("asset", ["stl", "cleats"])
@pytest.mark.parametrize("n", [4, 64])
@pytest.mark.parametrize("m", [1, 15, 17, 31, 33])
def test_twin_to_the_bit(gen, m, n, asset, task):
    cfg_of = lambda k: make_cfg(k, task=task, seed=5, cleats=asset == "cleats")
    inp = rows_of(gen, m)
    parent = _sim(cfg_of(n))
    qs = parent.query_state(m)
    fill(qs, inp)
    got = ask(qs, inp)
    twin = twin_of(cfg_of, inp)
    want = ask(twin, inp)
    assert got["tensors#0"].shape[1] == twin.num_bodies * 13 and got["tensors#1"].shape[1] == (twin.num_bodies - (task == "bez_kick")) * 144
    same_bits(got, want, what="M=%d N=%d %s %s" % (m, n, asset, task))
    qs.close(); twin.close(); parent.close()


def test_twin_without_a_ball_tensor_is_the_configs_ball_at_rest(gen):
    """bez_kick, ball=None: the config's ball_init pose at rest -- the state a freshly created sim has its ball in"""
    m = 17
    inp = rows_of(gen, m)
    parent = _sim(make_cfg(4, seed=5))
    qs = parent.query_state(m)
    qs.set(_dev(inp["root"]).view(m, 13), _dev(inp["dof"]).view(m, 18, 2))
    twin = _sim(make_cfg(m, seed=5))
    rs = _host(twin.refresh(abi.TENSOR_ROOT_STATE)).reshape(m, 2, 13)
    _write_states(twin, inp["root"], inp["dof"], rs[:, 1])          # (the ball rows as the reset left them)
    same_bits(ask(qs, inp), ask(twin, inp), what="ball at rest")
    qs.close(); twin.close(); parent.close()


# ---------------------------------------------------------------- 2. parameter gather

def random_params(n, seed):
    rng = np.random.default_rng(seed)
    lower, upper = np.asarray(abi_limits()[0]), np.asarray(abi_limits()[1])
    return {abi.PARAM_MASS_SCALE: rng.uniform(0.5, 1.5, (n, 19)).astype(np.float32),
            abi.PARAM_GRAVITY: (np.array([0.0, 0.0, -9.81]) + rng.uniform(-2, 2, (n, 3))).astype(np.float32),
            abi.PARAM_DOF_LOWER: (lower + rng.uniform(0.0, 0.2, (n, 18))).astype(np.float32),
            abi.PARAM_DOF_UPPER: (upper - rng.uniform(0.0, 0.2, (n, 18))).astype(np.float32)}


def abi_limits():
    from tests.state_sets import DOF_LOWER, DOF_UPPER
    return DOF_LOWER, DOF_UPPER


@pytest.mark.parametrize("which", [abi.QUERY_PARAMS, (abi.PARAM_GRAVITY, abi.PARAM_DOF_LOWER)])
def test_parameter_rows_are_gathered_by_env_id(gen, which):
    n, m = 8, 33
    cfg_of = lambda k: make_cfg(k, seed=5)
    parent = _sim(cfg_of(n))
    defaults = {p: _host(parent.get_env_params(p)) for p in abi.QUERY_PARAMS}       # (nothing is set yet: the default rows)
    params = {p: rows for p, rows in random_params(n, 3).items() if p in which}
    for p, rows in params.items():
        parent.set_env_params(p, _dev(rows))
    rng = np.random.default_rng(9)
    ids = np.concatenate([rng.permutation(n), rng.integers(0, n, m - n)])              # a permutation, then repeats
    outside = np.array([2, 16, 17, 32])                                                # rows in three different tiles
    ids[outside] = [-1, n, n + 5, -7]
    inside = np.setdiff1d(np.arange(m), outside)
    inp = rows_of(gen, m)
    qs = parent.query_state(m)
    fill(qs, inp, ids)
    got = ask(qs, inp)
    # the twin: env i holds env ids[i]'s rows, the default rows where the id is outside; only the parameters the parent has
    rows = {p: np.where(((ids >= 0) & (ids < n))[:, None], v[np.clip(ids, 0, n - 1)], defaults[p][:1]) for p, v in params.items()}
    twin = twin_of(cfg_of, inp, rows)
    same_bits(got, ask(twin, inp), what="gather")
    # ids outside 0 .. N-1: exactly what env_ids=None gives those rows
    fill(qs, inp)
    nominal = ask(qs, inp)
    same_bits(got, nominal, outside, outside, what="outside ids")
    differ = [k for k in got if (_bits(got[k][inside]) != _bits(nominal[k][inside])).any()]
    assert any(k.startswith("id ") for k in differ) and any(k.startswith("ik 3") for k in differ)   # (the rows did reach the kernels)
    qs.close(); twin.close(); parent.close()


# ---------------------------------------------------------------- 3. capture

def stepped_parent(n, steps=6, **kw):
    sim = _sim(make_cfg(n, seed=11, **kw))
    sim.set_env_params(abi.PARAM_MASS_SCALE, _dev(random_params(n, 5)[abi.PARAM_MASS_SCALE]))
    sim.set_randomization(_dr_cfg(freq=2, sched=4))
    g = torch.Generator(device="cpu").manual_seed(3)
    for _ in range(steps):
        sim.step((torch.rand(n, 18, generator=g) * 2 - 1).to("cuda:0").contiguous())
    return sim


@pytest.mark.parametrize("asset", ["stl", "cleats"])
def test_capture_answers_as_the_live_envs_do(gen, asset):
    n, m = NMAX, 33
    parent = stepped_parent(n, cleats=asset == "cleats")
    live_inp = rows_of(gen, n)
    live = ask(parent, live_inp)
    whole = parent.query_state(n)                                                      # the identity
    whole.capture()
    same_bits(ask(whole, live_inp), live, what="identity capture")
    whole.close()
    rng = np.random.default_rng(13)
    ids = np.concatenate([rng.permutation(n)[:20], rng.integers(0, n, m - 20)])
    outside = np.array([0, 15, 16, 32])
    ids[outside] = [-1, n, -3, n + 1]
    inside = np.setdiff1d(np.arange(m), outside)
    before = rows_of(gen, np.arange(m)[::-1])                                          # what set() puts there first: other states
    qs = parent.query_state(m)
    fill(qs, before)
    inp = rows_of(gen, np.clip(ids, 0, n - 1))                                         # row i is asked with env ids[i]'s udot, targets, ...
    kept = ask(qs, inp)
    qs.capture(_ids(ids))
    got = ask(qs, inp)
    same_bits(got, live, inside, ids[inside], what="captured rows")
    same_bits(got, kept, outside, outside, what="rows with ids outside 0 .. N-1")
    assert (_bits(got["id False 7#0"][inside]) != _bits(kept["id False 7#0"][inside])).any()
    qs.close(); parent.close()


# ---------------------------------------------------------------- 4. the live sim is untouched

LIVE_TENSORS = (abi.TENSOR_ROOT_STATE, abi.TENSOR_DOF_STATE, abi.TENSOR_RIGID_BODY_STATE, abi.TENSOR_NET_CONTACT_FORCE, abi.TENSOR_OBS, abi.TENSOR_REW,
                abi.TENSOR_RESET, abi.TENSOR_PROGRESS)


def live_tensors(sim):
    return {w: _host(sim.refresh(w)) for w in LIVE_TENSORS}


def test_the_live_sim_is_untouched(gen):
    n, m, steps = 16, 33, 4
    plain, busy = stepped_parent(n, steps=0), stepped_parent(n, steps=0)
    inp, live_inp = rows_of(gen, m), rows_of(gen, n)
    g = torch.Generator(device="cpu").manual_seed(17)
    qs = busy.query_state(m)
    for step in range(steps):
        act = (torch.rand(n, 18, generator=g) * 2 - 1).to("cuda:0").contiguous()
        plain.step(act); busy.step(act)
        asked = ask(busy, live_inp)                     # a live query, before the query state is used ...
        fill(qs, inp, np.arange(m) % n)
        ask(qs, inp)
        qs.capture(_ids((np.arange(m) * 5 - 2) % (n + 3)))
        ask(qs, inp)
        same_bits(ask(busy, live_inp), asked, what="live query after query-state queries, step %d" % step)   # ... and right after
        a, b = live_tensors(plain), live_tensors(busy)
        for w in LIVE_TENSORS:
            assert a[w].tobytes() == b[w].tobytes(), "tensor %d differs after step %d" % (w, step)
    same_bits(ask(plain, live_inp), ask(busy, live_inp), what="live queries of the two sims")
    qs.close(); plain.close(); busy.close()


# ---------------------------------------------------------------- 5. known answer

def test_rigid_body_rows_against_the_fd_reference(gen):
    """Bars: tests/gpu_util._bars -- 3x the fp32 oracle's worst error on these states plus 2 fp32 ulps of the value."""
    m = 33
    inp = rows_of(gen, m)
    cfg = make_cfg(m, task="bez_walk", seed=5)
    fd = fd_reference(inp["root"], inp["dof"])
    bars = _bars(field_errors(oracle_rows(cfg, "f32", inp["root"], inp["dof"])[:, :NB], fd), fd)
    parent = _sim(make_cfg(4, task="bez_walk", seed=5))
    qs = parent.query_state(m)
    fill(qs, inp)
    rows = _host(qs.refresh(abi.TENSOR_RIGID_BODY_STATE)).reshape(m, NB, 13)
    err = field_errors(rows, fd)
    for name in err:
        over = err[name] > bars[name]
        print("QUERY_STATE_FD %s worst error %.3g, worst error / bar %.3g" % (name, err[name].max(), (err[name] / bars[name]).max()))
        assert not over.any(), (name, np.argwhere(over)[:4])
    qs.close(); parent.close()


# ---------------------------------------------------------------- 6. refusals and ownership

def refused(sim, rc):
    msg = sim.lib.bez_sim_last_error(sim.h)
    return rc == -1 and len(msg) > 0


def test_refusals(gen):
    sim, other = _sim(make_cfg(4, task="bez_walk", seed=5)), _sim(make_cfg(4, task="bez_walk", seed=5))
    lib, stream = sim.lib, sim._stream()
    h = C.c_void_p()
    for rows in (0, -3):
        assert refused(sim, lib.bez_query_state_create(sim.h, rows, C.byref(h))) and not h.value
    assert lib.bez_query_state_create(None, 4, C.byref(h)) == -1 and len(lib.bez_sim_last_error(None)) > 0
    qs, theirs = sim.query_state(5), other.query_state(5)
    inp = rows_of(gen, 5)
    root, dof, ball = (_dev(inp[k]) for k in ("root", "dof", "ball"))
    ptr = lambda t: C.c_void_p(t.data_ptr())
    assert refused(sim, lib.bez_query_state_set(sim.h, qs.qs, ptr(root), ptr(dof), ptr(ball), None, stream))         # a ball on walk
    assert refused(sim, lib.bez_query_state_set(sim.h, qs.qs, None, ptr(dof), None, None, stream))
    assert refused(sim, lib.bez_query_state_set(sim.h, None, ptr(root), ptr(dof), None, None, stream))
    assert refused(sim, lib.bez_query_state_capture(sim.h, qs.qs, None, stream))                                     # identity with M != N
    assert refused(sim, lib.bez_query_state_bind(sim.h, theirs.qs))                                                  # another sim's
    assert refused(sim, lib.bez_query_state_set(sim.h, theirs.qs, ptr(root), ptr(dof), None, None, stream))
    assert lib.bez_query_state_bind(sim.h, qs.qs) == 0
    assert refused(sim, lib.bez_query_state_destroy(sim.h, qs.qs))                                                   # the bound one
    assert lib.bez_query_state_bind(sim.h, None) == 0
    for mask in (1 << abi.QUERY_RIGID_BODY_STATE, 1 << abi.QUERY_JACOBIAN, 1 << abi.QUERY_MASS_MATRIX, 0, 8):
        assert refused(sim, lib.bez_query_state_refresh(sim.h, qs.qs, mask, stream))                                 # never acquired / no such bit
    qs.dynamics_tensor("jacobian")
    assert lib.bez_query_state_refresh(sim.h, qs.qs, 1 << abi.QUERY_JACOBIAN, stream) == 0
    assert refused(sim, lib.bez_query_state_refresh(sim.h, qs.qs, (1 << abi.QUERY_JACOBIAN) | (1 << abi.QUERY_MASS_MATRIX), stream))
    torch.cuda.synchronize()
    qs.close(); theirs.close()
    survivor = sim.query_state(3)            # closing the sim frees it; the object only forgets its handle
    sim.close(); other.close()
    assert survivor.qs is None
    survivor.close()


def test_device_memory_returns_and_a_sim_without_query_states_allocates_nothing(gen):
    m = 2048
    sim = _sim(make_cfg(64, seed=5))
    out = torch.zeros(64, 24, device="cuda:0")
    before_query = _free()
    sim.inverse_dynamics(out=out)            # the first live query of a sim that never made a query state: nothing is allocated
    assert _free() == before_query
    pick = np.arange(m) % NMAX
    inp = rows_of(gen, pick)
    dev, ids = {k: _dev(v) for k, v in inp.items()}, _ids(pick)
    gc.collect(); torch.cuda.empty_cache()
    free0 = _free()
    qs = sim.query_state(m)
    qs.set(dev["root"].view(m, 13), dev["dof"].view(m, 18, 2), dev["ball"].view(m, 13), ids)
    qs.inverse_dynamics(); qs.proximity(); qs.dynamics_tensor("mass_matrix"); qs.dynamics_tensor("jacobian")
    qs.refresh_dynamics_tensors(); qs.refresh(abi.TENSOR_RIGID_BODY_STATE)
    used = _free()
    qs.inverse_dynamics(); qs.proximity(); qs.capture(ids); qs.refresh_dynamics_tensors(); qs.refresh(abi.TENSOR_RIGID_BODY_STATE)
    assert _free() == used                   # after the first use nothing allocates
    qs.close()
    del qs
    gc.collect(); torch.cuda.empty_cache()
    assert _free() == free0
    sim.close()
