"""GPU: env snapshots (include/bez_sim.h "Env snapshots"; BezSim.snapshot, VecTask.save_state / load_state).  Every comparison is bit for
bit: a snapshot copies, nothing is recomputed.  "All outputs" of a sim are what _outputs() collects: obs, rew, reset, progress, timeout, the
refreshed root, DOF, rigid-body, contact-force, target, previous-velocity, feet and goal tensors, the episode counter (read through a probe
snapshot: no tensor shows it), randomize, nonfinite, the three episode tensors, every env-param row, and the actuator tensors where
BEZ_FLAG_DOF_FORCE is on -- one (N, words) int32 matrix per step, so that a subset of envs is a subset of rows."""
import ctypes as C
import gc

import numpy as np
import pytest
import torch

from bez_isaacgym_amd import abi
from tests.gpu_util import _dev, _dr_cfg, _free, _ids, _sim
from tests.sim_cfg import make_cfg

pytestmark = pytest.mark.gpu

REFRESHED = ("ROOT_STATE", "DOF_STATE", "RIGID_BODY_STATE", "NET_CONTACT_FORCE", "DOF_TARGET", "PREV_LIN_VEL", "FEET", "GOAL")
LIVE = ("OBS", "REW", "RESET", "PROGRESS", "TIMEOUT", "RANDOMIZE_BUF", "NONFINITE_COUNT")
PARAMS = range(7)
_CACHE = {}


def _words(t, n):
    """(n, words) int32 view of a per-env tensor whose rows of env e are contiguous"""
    return t.contiguous().view(torch.int32).view(n, -1)


def _outputs(sim, episode=True):
    """({name: (first, last) column}, (N, words) int32 numpy) of everything the sim shows of its envs"""
    n, parts = sim.num_envs, []
    for name in REFRESHED:
        parts.append((name, _words(sim.refresh(getattr(abi, "TENSOR_" + name)), n)))
    for name in LIVE:
        parts.append((name, _words(sim.tensor(getattr(abi, "TENSOR_" + name)), n)))
    parts.append(("END_BITS", _words(sim.episode_tensor(abi.EPISODE_END_BITS), n)))
    parts.append(("END_COUNTS", _words(sim.episode_tensor(abi.EPISODE_END_COUNTS).t(), n)))
    parts.append(("REWARD_TERMS", _words(sim.episode_tensor(abi.EPISODE_REWARD_TERMS).t(), n)))
    for p in PARAMS:
        parts.append(("PARAM_%d" % p, _words(sim.get_env_params(p), n)))
    if sim.dof_force_enabled:
        sim.refresh_actuator_tensors()
        for k in (abi.ACTUATOR_DOF_FORCE, abi.ACTUATOR_DRIVE_TORQUE, abi.ACTUATOR_STATUS):
            parts.append(("ACTUATOR_%d" % k, _words(sim.actuator_tensor(k), n)))
    if episode:
        if "_probe" not in sim.__dict__:
            sim._probe = sim.snapshot(n)
        sim._probe.save()
        parts.append(("EPISODE", sim._probe.state_dict()["episode"].t().contiguous().to(sim.device)))
    cols, at = {}, 0
    for name, t in parts:
        cols[name] = (at, at + t.shape[1])
        at += t.shape[1]
    torch.cuda.synchronize()
    return cols, torch.cat([t for _, t in parts], dim=1).cpu().numpy()


def _same(cols, got, want, what, rows=None):
    """asserts two output matrices (or their rows `rows`) equal, naming the first tensor that differs"""
    if rows is not None:
        got, want = got[rows], want[rows]
    if not np.array_equal(got, want):
        bad = [name for name, (a, b) in cols.items() if not np.array_equal(got[:, a:b], want[:, a:b])]
        raise AssertionError("%s: differs in %s" % (what, ", ".join(bad)))


def _actions(n, steps, seed, scale=1.0):
    rng = np.random.default_rng(seed)
    return [_dev(rng.uniform(-scale, scale, (n, 18)).astype(np.float32)).view(n, 18) for _ in range(steps)]


def _step(sim, act, dr):
    """one control step as a task drives it: with a randomisation the action noise is added in front (the observation noise rides in
    the step: abi.FLAG_OBS_NOISE_IN_STEP)"""
    if dr:
        if "_noisy" not in sim.__dict__:
            sim._noisy = torch.empty_like(act)
        act = sim.add_dr_noise(act, 1, out=sim._noisy)
    sim.step(act)


def _run(sim, batches, dr, episode=True):
    kept = []
    for act in batches:
        _step(sim, act, dr)
        cols, out = _outputs(sim, episode)
        kept.append(out)
    return cols, kept


CASES = {"kick40": dict(n=40), "kick80": dict(n=80), "cleats": dict(n=40, cleats=True), "walk": dict(n=40, task="bez_walk"),
         "dof_force": dict(n=40, flags=abi.FLAG_DOF_FORCE)}


def _dr_sim(case, seed=11):
    kw = dict(CASES[case])
    n, flags = kw.pop("n"), kw.pop("flags", 0)
    cfg = make_cfg(n, seed=seed, **kw)
    cfg.max_episode_length = 25
    cfg.flags |= flags | abi.FLAG_OBS_NOISE_IN_STEP
    sim = _sim(cfg)
    sim.set_randomization(_dr_cfg(freq=3, sched=40))
    return sim


def _mass_rows(n):
    return _dev(np.random.default_rng(3).uniform(0.8, 1.2, (n, 19)).astype(np.float32))


def _kept(case):
    """sim A of a case after 30 + 40 steps, its snapshot of step 30, the 40 action batches and A's outputs after each of them: computed
    once per case, shared by the rewind and the twin test and left unchanged"""
    if case not in _CACHE:
        a = _dr_sim(case)
        n = a.num_envs
        a.set_env_params(abi.PARAM_MASS_SCALE, _mass_rows(n))
        for act in _actions(n, 30, 1):
            _step(a, act, True)
        snap = a.snapshot(n)
        snap.save()
        batches = _actions(n, 40, 2)
        cols, kept = _run(a, batches, True)
        resets = sum(int(k[:, slice(*cols["RESET"])].any()) for k in kept)
        moved = any(not np.array_equal(kept[0][:, slice(*cols["PARAM_%d" % p])], kept[-1][:, slice(*cols["PARAM_%d" % p])]) for p in PARAMS)
        assert resets >= 1 and moved, "the kept window must contain a reset and a change of a parameter row (%d, %s)" % (resets, moved)
        _CACHE[case] = (a, snap, batches, cols, kept)
    return _CACHE[case]


@pytest.mark.parametrize("case", list(CASES))
def test_rewind(case):
    """save, 40 steps, restore with GLOBALS, the same 40 batches: every output of every step again -- through resets, horizon
    time-outs, redraws of the parameter rows, the moving noise parameters and (bez_walk) the goal draw keyed by the device counter"""
    a, snap, batches, cols, kept = _kept(case)
    snap.restore(globals_=True)
    _, again = _run(a, batches, True)
    for t, (g, w) in enumerate(zip(again, kept)):
        _same(cols, g, w, "%s step %d" % (case, t))


@pytest.mark.parametrize("case", ["kick40", "walk"])
def test_twin(case):
    """a second sim of the same config that was never stepped, and has no mass-scale rows of its own, continues as A did"""
    a, snap, batches, cols, kept = _kept(case)
    b = _dr_sim(case)
    snap.restore(b, globals_=True)
    _, again = _run(b, batches, True)
    for t, (g, w) in enumerate(zip(again, kept)):
        _same(cols, g, w, "%s twin step %d" % (case, t))
    b.close()


def test_untouched():
    """saving, exporting and importing between the steps changes nothing in the sim that does it"""
    plain, busy = _dr_sim("kick40", seed=5), _dr_sim("kick40", seed=5)
    snap = busy.snapshot(40)
    for t, act in enumerate(_actions(40, 12, 4)):
        _step(plain, act, True); _step(busy, act, True)
        snap.save()
        snap.load_state_dict(snap.state_dict())
        cols, want = _outputs(plain, episode=False)
        _, got = _outputs(busy, episode=False)
        _same(cols, got, want, "step %d" % t)
    plain.close(); busy.close()


def _dict_of(sim, snap=None):
    snap = snap or sim.snapshot(sim.num_envs)
    snap.save()
    return {k: v.numpy() for k, v in snap.state_dict().items()}


SECTIONS = abi.SNAPSHOT_SECTIONS


def test_partial_restore():
    """N = 80, no randomisation, small actions from the reset pose.  The save is taken after three steps, not at creation: a restore
    without GLOBALS leaves the sim's count of observation passes alone, and only the very first pass of a sim differs from the later
    ones (it sees a zero previous velocity), so the kept window must lie behind it to be repeatable by a partial restore."""
    n, S = 80, [1, 17, 40, 79]
    sim = _sim(make_cfg(n, seed=8))
    for act in _actions(n, 3, 5, 0.1):
        sim.step(act)
    first, second = sim.snapshot(n), sim.snapshot(n)
    first.save()
    saved = {k: v.numpy() for k, v in first.state_dict().items()}
    batches = _actions(n, 10, 6, 0.1)
    cols, kept = _run(sim, batches, False)
    assert not any(k[S, slice(*cols["RESET"])].any() for k in kept), "no env of S may reset in the kept window"
    before = _dict_of(sim, second)
    first.restore(env_ids=_ids(S + [-1, n]), row_ids=_ids(S + [3, 5]))
    after = _dict_of(sim, second)
    others = [e for e in range(n) if e not in S]
    for name in SECTIONS:
        assert np.array_equal(after[name][:, S], saved[name][:, S]), name
        assert np.array_equal(after[name][:, others], before[name][:, others]), name
    assert not np.array_equal(after["state"][:, S], before["state"][:, S])
    assert np.array_equal(after["globals"], before["globals"])
    _, again = _run(sim, batches, False)
    for t, (g, w) in enumerate(zip(again, kept)):
        _same(cols, g, w, "step %d" % t, rows=S)
    sim.close()


def test_fan_out_into_another_sim():
    """row e of A (N = 64) into envs e and e + 64 of D (N = 128, another seed): whole-tile moves, which the step kernels are neutral to"""
    a, d = _sim(make_cfg(64, seed=8)), _sim(make_cfg(128, seed=99))
    for act in _actions(64, 3, 5, 0.1):
        a.step(act)
    snap = a.snapshot(64)
    snap.save()
    batches = _actions(64, 10, 6, 0.1)
    cols, kept = _run(a, batches, False, episode=False)
    assert not any(k[:, slice(*cols["RESET"])].any() for k in kept), "no reset in the kept window"
    env_ids, row_ids = _ids(np.arange(128)), _ids(np.arange(128) % 64)
    snap.restore(d, env_ids=env_ids, row_ids=row_ids, globals_=True)
    _, again = _run(d, [torch.cat([b, b]) for b in batches], False, episode=False)
    for t, (g, w) in enumerate(zip(again, kept)):
        _same(cols, g[:64], w, "first half, step %d" % t)
        _same(cols, g[64:], w, "second half, step %d" % t)
    snap.restore(d, env_ids=env_ids, row_ids=row_ids, globals_=True)
    _, other = _run(d, [torch.cat([b, -b]) for b in batches], False, episode=False)
    _same(cols, other[-1][:64], kept[-1], "first half with other actions behind it")
    assert not np.array_equal(other[-1][64:, slice(*cols["DOF_STATE"])], kept[-1][:, slice(*cols["DOF_STATE"])])
    # a random permutation with repeats, by read-back
    pick = np.random.default_rng(7).integers(0, 64, 128)
    snap.restore(d, row_ids=_ids(pick), count=128)
    rows, got = {k: v.numpy() for k, v in snap.state_dict().items()}, _dict_of(d)
    for name in SECTIONS:
        assert np.array_equal(got[name], rows[name][:, pick]), name
    a.close(); d.close()


@pytest.mark.parametrize("m", [1, 17, 64])
def test_rows_and_ids(m):
    n = 40
    sim = _sim(make_cfg(n, seed=8))
    for act in _actions(n, 4, 5):
        sim.step(act)
    full = _dict_of(sim)
    pick = np.random.default_rng(m).integers(0, n, m)
    snap = sim.snapshot(m)
    snap.save(_ids(pick))
    got = {k: v.numpy() for k, v in snap.state_dict().items()}
    for name in SECTIONS:
        assert np.array_equal(got[name], full[name][:, pick]), name
    sim.step(_actions(n, 1, 6)[0])                      # the envs move on; rows with an id outside 0 .. N-1 keep the first save
    later = _dict_of(sim)
    out = np.arange(m) % 2 == 0
    snap.save(_ids(np.where(out, np.where(np.arange(m) % 4 == 0, -1, n), pick)))
    again = {k: v.numpy() for k, v in snap.state_dict().items()}
    for name in SECTIONS:
        assert np.array_equal(again[name][:, out], got[name][:, out]), name
        assert np.array_equal(again[name][:, ~out], later[name][:, pick[~out]]), name
    assert not np.array_equal(later["state"], full["state"])
    # a restore whose row id is out of range skips the entry
    snap.restore(env_ids=_ids([0, 1, 2]), row_ids=_ids([0, m, -1]))
    now = _dict_of(sim)
    for name in SECTIONS:
        assert np.array_equal(now[name][:, 0], again[name][:, 0]), name
        assert np.array_equal(now[name][:, 1:], later[name][:, 1:]), name
    sim.close()


def _stepped_dr_sim():
    a = _dr_sim("kick40", seed=5)
    a.set_env_params(abi.PARAM_MASS_SCALE, _mass_rows(40))
    for act in _actions(40, 8, 4):
        _step(a, act, True)
    return a


def test_export_import():
    a, b, c = _stepped_dr_sim(), _dr_sim("kick40", seed=5), _dr_sim("kick40", seed=5)
    sa, sc = a.snapshot(40), c.snapshot(40)
    sa.save()
    sa.restore(b, globals_=True)                        # directly ...
    d = sa.state_dict()
    assert all(t.device.type == "cpu" and t.dtype == torch.int32 for t in d.values()) and int(d["header"][0]) == abi.SNAPSHOT_MAGIC
    sc.load_state_dict(d)                               # ... and by way of the host
    sc.restore(globals_=True)
    db, dc = _dict_of(b), _dict_of(c)
    for name in db:
        assert np.array_equal(db[name], dc[name]), name
    act = _actions(40, 1, 9)[0]
    _step(b, act, True); _step(c, act, True)
    cols, ob = _outputs(b)
    _same(cols, _outputs(c)[1], ob, "one step after the restore")
    # blobs that do not fit: rc -1, and the snapshot is as it was
    from bez_isaacgym_amd.sim import BezSimError
    kept = sc.state_dict()
    small = a.snapshot(39)
    small.save(_ids(np.arange(39)))
    version = dict(d, header=d["header"].clone())
    version["header"][1] = abi.SNAPSHOT_LAYOUT + 1
    for bad, why in ((small.state_dict(), "rows"), (version, "layout version")):
        with pytest.raises(BezSimError, match=why):
            sc.load_state_dict(bad)
    blob = torch.cat([d[k].reshape(-1) for k in ("header",) + SECTIONS + ("globals",)]).contiguous()
    for nbytes in (blob.numel() * 4 - 4, abi.SNAPSHOT_HEADER_WORDS * 4, 12):
        assert c.lib.bez_snapshot_import(c.h, sc.snap, C.c_void_p(blob.data_ptr()), nbytes, None) == -1
        assert b"truncated" in c.lib.bez_sim_last_error(c.h)
    now = sc.state_dict()
    assert all(torch.equal(now[k], kept[k]) for k in kept)
    for s in (a, b, c):
        s.close()


def test_parameter_presence():
    n, S = 40, [2, 9, 33]
    rng = np.random.default_rng(12)
    mass, grav = rng.uniform(0.8, 1.2, (n, 19)).astype(np.float32), (np.array([0, 0, -9.81]) + rng.uniform(-1, 1, (n, 3))).astype(np.float32)
    kp = rng.uniform(0.5, 1.5, (n, 18)).astype(np.float32)
    src = _sim(make_cfg(n, seed=8))
    src.set_env_params(abi.PARAM_MASS_SCALE, _dev(mass)); src.set_env_params(abi.PARAM_GRAVITY, _dev(grav))
    for act in _actions(n, 3, 5, 0.3):
        src.step(act)
    snap = src.snapshot(n)
    snap.save()
    ids = _ids(S)
    act = _actions(n, 1, 6, 0.3)[0]

    # the snapshot has mass-scale and gravity rows, the destination none: its rows on the restored envs, the defaults elsewhere
    dst, twin = _sim(make_cfg(n, seed=8)), _sim(make_cfg(n, seed=8))
    snap.restore(dst, env_ids=ids, row_ids=ids)
    want_mass, want_grav = np.ones((n, 19), np.float32), np.tile(np.array(list(dst.cfg.gravity), np.float32), (n, 1))
    want_mass[S], want_grav[S] = mass[S], grav[S]
    assert np.array_equal(dst.get_env_params(abi.PARAM_MASS_SCALE).cpu().numpy(), want_mass)
    assert np.array_equal(dst.get_env_params(abi.PARAM_GRAVITY).cpu().numpy(), want_grav)
    snap.restore(twin, env_ids=ids, row_ids=ids)
    twin.set_env_params(abi.PARAM_MASS_SCALE, _dev(want_mass)); twin.set_env_params(abi.PARAM_GRAVITY, _dev(want_grav))
    dst.step(act); twin.step(act)
    cols, got = _outputs(dst)
    _same(cols, got, _outputs(twin)[1], "mass and gravity rows by the restore against set_env_params")
    dst.close(); twin.close()

    # the destination has stiffness rows, the snapshot none: the restored envs read the default, and the packed copy follows
    dst, twin = _sim(make_cfg(n, seed=8)), _sim(make_cfg(n, seed=8))
    dst.set_env_params(abi.PARAM_KP_SCALE, _dev(kp))
    snap.restore(dst, env_ids=ids, row_ids=ids)
    want_kp = kp.copy()
    want_kp[S] = 1.0
    assert np.array_equal(dst.get_env_params(abi.PARAM_KP_SCALE).cpu().numpy(), want_kp)
    snap.restore(twin, env_ids=ids, row_ids=ids)
    twin.set_env_params(abi.PARAM_KP_SCALE, _dev(want_kp))
    dst.step(act); twin.step(act)
    cols, got = _outputs(dst)
    _same(cols, got, _outputs(twin)[1], "stiffness rows: defaults by the restore against set_env_params")
    stale = _sim(make_cfg(n, seed=8))                   # (the check can fail: with the rows the restore replaced, the step differs)
    stale.set_env_params(abi.PARAM_KP_SCALE, _dev(kp))
    snap.restore(stale, env_ids=ids, row_ids=ids)
    stale.set_env_params(abi.PARAM_KP_SCALE, _dev(kp))
    stale.step(act)
    assert not np.array_equal(_outputs(stale)[1][S], got[S])
    for s in (src, dst, twin, stale):
        s.close()


def test_refusals():
    a, other = _sim(make_cfg(40, seed=8)), _sim(make_cfg(40, seed=8))
    walk, cleats = _sim(make_cfg(40, seed=8, task="bez_walk")), _sim(make_cfg(40, seed=8, cleats=True))
    lib, h = a.lib, C.c_void_p()
    both = abi.SNAPSHOT_ENVS | abi.SNAPSHOT_GLOBALS

    def refused(rc, sim, word):
        msg = lib.bez_sim_last_error(sim.h).decode()
        assert rc == -1 and word in msg, (rc, msg)

    refused(lib.bez_snapshot_create(a.h, 0, C.byref(h)), a, "rows")
    refused(lib.bez_snapshot_create(a.h, -3, C.byref(h)), a, "rows")
    snap, empty = a.snapshot(17), a.snapshot(17)
    refused(lib.bez_snapshot_restore(a.h, empty.snap, None, None, 17, both, None), a, "nothing was saved")
    snap.save(_ids(np.arange(17)))
    refused(lib.bez_snapshot_save(a.h, None, None, None), a, "null")
    refused(lib.bez_snapshot_restore(a.h, None, None, None, 1, both, None), a, "null")
    refused(lib.bez_snapshot_save(other.h, snap.snap, None, None), other, "another sim")
    refused(lib.bez_snapshot_destroy(other.h, snap.snap), other, "another sim")
    size = C.c_int64(0)
    refused(lib.bez_snapshot_export(other.h, snap.snap, None, C.byref(size), None), other, "another sim")
    refused(lib.bez_snapshot_restore(a.h, snap.snap, None, None, -1, both, None), a, "count")
    refused(lib.bez_snapshot_restore(a.h, snap.snap, None, None, 18, both, None), a, "count")
    for what in (0, 4, both | 4, abi.SNAPSHOT_GLOBALS):
        refused(lib.bez_snapshot_restore(a.h, snap.snap, None, None, 17, what, None), a, "what")
    refused(lib.bez_snapshot_restore(walk.h, snap.snap, None, None, 17, both, None), walk, "task")
    refused(lib.bez_snapshot_restore(cleats.h, snap.snap, None, None, 17, both, None), cleats, "asset")
    assert lib.bez_snapshot_restore(other.h, snap.snap, None, None, 17, both, None) == 0   # (another sim of the same kind is fine)
    dead = C.c_void_p(empty.snap.value)
    empty.close()
    refused(lib.bez_snapshot_save(a.h, dead, None, None), a, "not alive")
    refused(lib.bez_snapshot_restore(a.h, dead, None, None, 1, both, None), a, "not alive")
    refused(lib.bez_snapshot_destroy(a.h, dead), a, "not alive")
    theirs = C.c_void_p(snap.snap.value)
    a.close()                                           # the sim takes its snapshots with it
    assert snap.snap is None
    refused(lib.bez_snapshot_restore(other.h, theirs, None, None, 1, both, None), other, "not alive")
    for s in (other, walk, cleats):
        s.close()


def test_device_memory():
    n = 1024
    ids = _ids(np.arange(n)[::-1].copy())
    gc.collect(); torch.cuda.empty_cache()
    start = _free()
    plain = _sim(make_cfg(n, seed=5))                   # never makes a snapshot
    plain_cost = start - _free()
    plain.close()
    gc.collect(); torch.cuda.empty_cache()
    assert _free() == start
    sim = _sim(make_cfg(n, seed=5))
    assert start - _free() == plain_cost                # what a sim allocates at creation does not know of snapshots
    sim.set_env_params(abi.PARAM_KP_SCALE, _dev(np.ones((n, 18), np.float32)))
    act = _actions(n, 1, 3)[0]
    sim.step(act)
    free0 = _free()
    snap = sim.snapshot(n)
    snap.save(); snap.restore(globals_=True); snap.save(ids); snap.restore(env_ids=ids, row_ids=ids)
    used = _free()
    assert used < free0
    for _ in range(3):
        snap.save(); sim.step(act); snap.restore(globals_=True); snap.save(ids); snap.restore(env_ids=ids)
    assert _free() == used                              # after the first save and restore nothing allocates
    snap.close()
    snap.close()
    del snap
    gc.collect(); torch.cuda.empty_cache()
    assert _free() == free0
    sim.close()


@pytest.mark.parametrize("lean", [True, False])
def test_vec_task_save_and_load_state(lean):
    """save_state, five steps, load_state, the same five steps: what the task shows is the first pass again after every step.  While
    the env steps lean, net_contact_forces refuses to be read (KickEnv._not_lean), so it is compared in the non-lean case only."""
    from bez_isaacgym_amd.utils.config import load_config
    from bez_isaacgym_amd.utils.rlgames_utils import get_rlgames_env_creator
    cfg = load_config(["task=bez_kick", "num_envs=16", "headless=True"])
    cfg["task"]["seed"] = 42
    env = get_rlgames_env_creator(cfg["task"], "bez_kick", "cuda:0", "cuda:0", 0, True)()
    n = env.num_envs
    batches = _actions(n, 7, 21)
    for act in batches[:2]:
        env.step(act)
    env.set_lean(lean)
    env.step(batches[2])                                 # (lean stepping starts with the step after the switch)

    def shown():
        names = ["obs_buf", "rew_buf", "reset_buf", "progress_buf", "root_states", "dof_state"] + ([] if lean else ["net_contact_forces"])
        torch.cuda.synchronize()
        return {k: getattr(env, k).detach().cpu().numpy().copy() for k in names}

    def run():
        out = []
        for act in batches[2:]:
            obs, rew, reset, extras = env.step(act)
            out.append(dict(shown(), obs=obs["obs"].cpu().numpy().copy(), time_outs=extras["time_outs"].cpu().numpy().copy()))
        return out

    snap = env.save_state()
    before = shown()
    first = run()
    env.load_state(snap)
    now = shown()                                       # straight after the load the accessors show the saved envs
    assert all(np.array_equal(now[k].view(np.uint32), before[k].view(np.uint32)) for k in before)
    assert env.last_step == snap.host["last_step"]
    qs = env.query_state()                              # a query state made now captures the restored envs
    qs.capture()
    assert torch.equal(qs.sim.refresh(abi.TENSOR_RIGID_BODY_STATE), env.rigid_body)
    qs.close()
    second = run()
    for t, (f, s) in enumerate(zip(first, second)):
        for k in f:
            assert np.array_equal(f[k].view(np.uint32) if f[k].dtype == np.float32 else f[k], s[k].view(np.uint32) if s[k].dtype == np.float32 else s[k]), (t, k)
    assert not np.array_equal(first[-1]["dof_state"], before["dof_state"])   # (the envs did move in between)
    snap.close()
    env.sim.close()
