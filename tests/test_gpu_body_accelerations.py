"""GPU: bez_sim_body_accelerations (include/bez_sim.h "Body accelerations": J_b udot + Jdot_b u - g of every rigid body, rows [acceleration
of the body's origin; angular acceleration]) against the fp64 reference of tests/body_accel_numpy.py, against the Jacobian tensor, and
against its own contract to the bit.

Sizes: 1, 63, 64, 65, 300 and, around the kernel's 16-env tile, 15, 16, 17.  No outlier budget anywhere: every element of every env is
held to its bar.

  known answer   per block (rows 0:3, rows 3:6), each of UDOT, VELOCITY, GRAVITY, MOTION, ALL in both spaces: 3x the worst absolute error
                 of the fp32 yardstick (the worse of acc_ref and acc_ref_world evaluated in np.float32 against fp64) on the same states
                 + 2 fp32 ulps of the block's largest |reference|.
  J udot         body_accelerations(udot, ACC_UDOT) against the refreshed Jacobian times udot, both fp32 on the GPU: per element the
                 fp64-evaluated bound of the 24-term fp32 dot product, 24 * 2^-23 * sum_j |J_ij| |udot_j|, + the known-answer bar.
  exact          every bit-level statement of the header.

Measured on MI355X: see DESIGN.md 4.3i."""
import ctypes as C

import numpy as np
import pytest
import torch

from bez_isaacgym_amd import abi
from tests import body_accel_numpy as BA
from tests.gpu_util import ASSETS, _bits, _dev, _free, _host, _sim, _write_states
from tests.sim_cfg import make_cfg
from tests.state_sets import ball_states, generate_states, ulp32

pytestmark = pytest.mark.gpu

TILE = 16
SIZES = (1, TILE - 1, TILE, TILE + 1, 63, 64, 65, 300)
NMAX = max(SIZES)
NG = abi.NUM_GEN
TERMS = (abi.ACC_UDOT, abi.ACC_VELOCITY, abi.ACC_GRAVITY, abi.ACC_MOTION, abi.ACC_ALL)
SPACES = (abi.SPACE_ENV, abi.SPACE_LOCAL)
_CACHE = {}


def _states():
    if "states" not in _CACHE:
        root, dof, _ = generate_states(NMAX)
        rng = np.random.default_rng(37)
        udot = rng.uniform(-10, 10, (NMAX, NG)).astype(np.float32)   # O(10) in mixed SI units: m/s^2, rad/s^2
        gravity = (np.array([0.0, 0.0, -9.81]) + rng.uniform(-2, 2, (NMAX, 3))).astype(np.float32)
        _CACHE["states"] = dict(root=root, dof=dof, ball=ball_states(NMAX), udot=udot, gravity=gravity)
    return _CACHE["states"]


def _refs(asset, randomized, cfg):
    """{(terms, space): (fp64 reference (NMAX, NB, 6), bar (6,))} of an asset's link model; computed once per key and left unchanged"""
    key = ("ref", "cleats" if asset == "cleats" else "stl", randomized)
    if key not in _CACHE:
        st = _states()
        g = st["gravity"] if randomized else np.asarray(list(cfg.gravity), np.float64)
        model = BA.model_of(asset)
        out = {}
        for terms in TERMS:
            for space in SPACES:
                r64 = BA.acc_ref(model, st["root"], st["dof"], st["udot"], g, terms, space)
                e32 = BA.yardstick_error(model, st["root"], st["dof"], st["udot"], g, terms, space, r64)
                bar = np.zeros(6)
                for k, (_, sl) in enumerate(BA.BLOCKS):
                    bar[sl] = 3.0 * e32[k] + 2.0 * float(ulp32(np.abs(r64[:, :, sl]).max()))
                out[terms, space] = (r64, bar)
        _CACHE[key] = out
    return _CACHE[key]


def _call(sim, udot, terms, space=abi.SPACE_ENV):
    return _host(sim.body_accelerations(udot, terms, space))


def _nb(sim):
    return sim.num_bodies - (1 if sim.has_ball else 0)


def _prepared(cfg, n, randomized):
    st = _states()
    sim = _sim(cfg)
    _write_states(sim, st["root"][:n], st["dof"][:n], st["ball"][:n])
    if randomized:
        sim.set_env_params(abi.PARAM_GRAVITY, _dev(st["gravity"][:n]))
    return sim, _dev(st["udot"][:n]).view(n, NG)


@pytest.mark.parametrize("randomized", [False, True], ids=["default_params", "gravity_rows"])
@pytest.mark.parametrize("task", ["bez_kick", "bez_walk"])
@pytest.mark.parametrize("asset", list(ASSETS))
def test_known_answer(asset, task, randomized):
    """each of UDOT, VELOCITY, GRAVITY, MOTION and ALL in both spaces against acc_ref in fp64 on the fp32 states, every element of every
    env, with the config's gravity and with a different BEZ_PARAM_GRAVITY row per env"""
    cfg = lambda n: make_cfg(n, task=task, seed=5, **ASSETS[asset])
    refs = _refs(asset, randomized, cfg(1))
    report = {}
    for n in SIZES:
        sim, udot = _prepared(cfg(n), n, randomized)
        for terms in TERMS:
            for space in SPACES:
                ref, bar = refs[terms, space]
                got = _call(sim, udot, terms, space)
                assert got.shape == (n, ref.shape[1], 6) and got.dtype == np.float32
                err = np.abs(got.astype(np.float64) - ref[:n])
                for name, sl in BA.BLOCKS:
                    key = (terms, "local" if space else "env", name)
                    report[key] = max(report.get(key, 0.0), float((err[:, :, sl] / bar[sl]).max()))
        sim.close()
    print("ACC_KNOWN_ANSWER worst error / bar {(terms, space, block)}:", asset, task, "randomized" if randomized else "default",
          {k: round(v, 3) for k, v in report.items()}, "bars (all terms, env):", [float(refs[abi.ACC_ALL, abi.SPACE_ENV][1][sl][0]) for _, sl in BA.BLOCKS])
    assert max(report.values()) <= 1.0, report


@pytest.mark.parametrize("asset", list(ASSETS))
def test_udot_term_is_the_jacobian_times_udot(asset):
    """both sides fp32 on the GPU"""
    st = _states()
    cfg = lambda n: make_cfg(n, seed=5, **ASSETS[asset])
    bar = _refs(asset, False, cfg(1))[abi.ACC_UDOT, abi.SPACE_ENV][1]
    worst = 0.0
    for n in SIZES:
        sim, udot = _prepared(cfg(n), n, False)
        Jt = sim.dynamics_tensor("jacobian")
        sim.refresh_dynamics_tensors("jacobian")
        J = _host(Jt).astype(np.float64).reshape(n, -1, 6, NG)
        got = _call(sim, udot, abi.ACC_UDOT).astype(np.float64)
        sim.close()
        ud = st["udot"][:n].astype(np.float64)
        want = np.einsum("ebij,ej->ebi", J, ud)
        tol = NG * 2.0 ** -23 * np.einsum("ebij,ej->ebi", np.abs(J), np.abs(ud)) + bar
        ratio = np.abs(got - want) / tol
        worst = max(worst, float(ratio.max()))
        assert (ratio <= 1.0).all(), (asset, n, float(ratio.max()), [tuple(x) for x in np.argwhere(ratio > 1)[:5]])
    print("ACC_VS_JACOBIAN worst |UDOT term - J udot| / tolerance:", asset, round(worst, 3))


@pytest.mark.parametrize("asset", list(ASSETS))
def test_exact_structure(asset):
    """every bit-level statement of the header: +0.0f where an input is dropped or vanishes, 0 - g, the terms as fp32 sums of the
    single-term calls, the torso's rows"""
    st = _states()
    n = 65
    cfg = make_cfg(n, seed=5, **ASSETS[asset])
    sim, udot = _prepared(cfg, n, True)
    g = st["gravity"][:n]
    zero = lambda a: not _bits(a).any()     # +0.0f to the bit
    parts = {}
    for space in SPACES:
        assert zero(_call(sim, None, abi.ACC_UDOT, space))                       # udot_dev = NULL
        grav = _call(sim, udot, abi.ACC_GRAVITY, space)
        assert zero(grav[:, :, 3:6])
        if space == abi.SPACE_ENV:
            want = np.broadcast_to((np.float32(0) - g)[:, None, :], grav[:, :, 0:3].shape)
            np.testing.assert_array_equal(_bits(grav[:, :, 0:3]), _bits(want))
            parts = {t: _call(sim, udot, t) for t in TERMS}
            np.testing.assert_array_equal(_bits(parts[abi.ACC_MOTION]), _bits(parts[abi.ACC_UDOT] + parts[abi.ACC_VELOCITY]))
            np.testing.assert_array_equal(_bits(parts[abi.ACC_ALL]), _bits((parts[abi.ACC_UDOT] + parts[abi.ACC_VELOCITY]) + parts[abi.ACC_GRAVITY]))
            np.testing.assert_array_equal(_bits(parts[abi.ACC_UDOT][:, 0]), _bits(st["udot"][:n, 0:6]))   # the torso: udot[0:6] ...
            assert zero(parts[abi.ACC_VELOCITY][:, 0])                                                     # ... and no bias acceleration
            assert np.abs(parts[abi.ACC_VELOCITY][:, 1:]).max() > 10 and parts[abi.ACC_UDOT].dtype == np.float32
    root, dof = st["root"][:n].copy(), st["dof"][:n].copy()
    root[:, 7:13] = 0; dof[:, :, 1] = 0
    _write_states(sim, root, dof, st["ball"][:n])
    sim.set_env_params(abi.PARAM_GRAVITY, _dev(np.zeros((n, 3), np.float32)))
    for space in SPACES:
        assert zero(_call(sim, udot, abi.ACC_VELOCITY, space))                   # u = 0
        assert zero(_call(sim, udot, abi.ACC_GRAVITY, space))                    # a zero gravity row
    np.testing.assert_array_equal(_bits(_call(sim, udot, abi.ACC_ALL)), _bits(parts[abi.ACC_UDOT]))   # ... and what is left is the UDOT term
    sim.close()


def test_contract():
    """bad `terms`, a bad `space` and a null out: rc -1 with a message that names the function; ten calls allocate nothing; the sim's state
    is untouched; a side stream and an out view one float off 16-byte alignment give the same bits; the Python layer checks what it is
    handed"""
    from bez_isaacgym_amd.sim import BezSimError
    n = 65
    sim, udot = _prepared(make_cfg(n, seed=2), n, False)
    nb = _nb(sim)
    out = torch.zeros(n, nb, 6, device="cuda:0")
    torch.cuda.synchronize()
    po = C.c_void_p(out.data_ptr())
    raw = lambda terms, space, o: sim.lib.bez_sim_body_accelerations(sim.h, C.c_void_p(udot.data_ptr()), terms, space, o, None)
    for terms, space, o in ((0, 0, po), (8, 0, po), (1 << 31, 0, po), (9, 1, po), (abi.ACC_ALL, 2, po), (abi.ACC_ALL, -1, po), (abi.ACC_ALL, 0, None)):
        assert raw(terms, space, o) == -1, (terms, space)
        assert b"bez_sim_body_accelerations" in sim.lib.bez_sim_last_error(sim.h)
    assert sim.lib.bez_sim_body_accelerations(None, None, abi.ACC_ALL, 0, po, None) == -1
    assert b"bez_sim_body_accelerations" in sim.lib.bez_sim_last_error(None)
    assert not out.any()
    snap = lambda: [_host(sim.refresh(w)) for w in (abi.TENSOR_ROOT_STATE, abi.TENSOR_DOF_STATE, abi.TENSOR_DOF_TARGET)]
    state = snap()
    want = _call(sim, udot, abi.ACC_ALL, abi.SPACE_LOCAL)
    before = _free()
    for k in range(10):
        sim.body_accelerations(udot if k % 2 else None, TERMS[k % 5], SPACES[k % 2], out if k % 3 else None)
    assert _free() == before
    for a, b in zip(state, snap()):
        np.testing.assert_array_equal(_bits(a), _bits(b))
    assert raw(abi.ACC_ALL, abi.SPACE_LOCAL, po) == 0
    np.testing.assert_array_equal(_bits(_host(out)), _bits(want))
    out.zero_()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        sim.body_accelerations(udot, abi.ACC_ALL, "local", out)
    np.testing.assert_array_equal(_bits(_host(out)), _bits(want))
    assert np.abs(want).max() > 10
    # views that are contiguous but only 4-byte aligned take the kernel's scalar paths: same bits, and not a float outside the view
    pad = torch.full((n * nb * 6 + 2,), -7.0, device="cuda:0")
    pad_u, pad_o = torch.zeros(n * NG + 1, device="cuda:0"), pad[1:-1].view(n, nb, 6)
    pad_u[1:] = udot.reshape(-1)
    sim.body_accelerations(pad_u[1:].view(n, NG), abi.ACC_ALL, abi.SPACE_LOCAL, pad_o)
    np.testing.assert_array_equal(_bits(_host(pad_o)), _bits(want))
    assert _host(pad)[0] == -7.0 and _host(pad)[-1] == -7.0
    for bad in (dict(udot=udot[:, :23]), dict(udot=udot.double()), dict(udot=udot.cpu()), dict(udot=udot.t().contiguous().t()), dict(out=out[:-1]),
                dict(out=out.reshape(-1)), dict(out=out[:, :, :3]), dict(udot=_host(udot)), dict(terms=0), dict(terms=16)):
        with pytest.raises(BezSimError):
            sim.body_accelerations(**bad)
    with pytest.raises(ValueError):
        sim.body_accelerations(space="world")
    sim.close()


@pytest.mark.parametrize("n", [64, 65])
def test_the_last_tile_ends_where_the_output_ends(n):
    """rows of 126 floats: an odd number of envs leaves a part-filled last float4, which the scalar tail writes and nothing overruns"""
    sim, udot = _prepared(make_cfg(n, task="bez_walk", seed=2), n, False)
    nb = _nb(sim)
    want = _call(sim, udot, abi.ACC_MOTION)
    buf = torch.full((n * nb * 6 + 8,), -7.0, device="cuda:0")
    sim.body_accelerations(udot, abi.ACC_MOTION, abi.SPACE_ENV, buf[: n * nb * 6].view(n, nb, 6))
    got = _host(buf)
    np.testing.assert_array_equal(_bits(got[: n * nb * 6]), _bits(want.reshape(-1)))
    assert (got[n * nb * 6:] == -7.0).all() and (n * nb * 6) % 4 == (0 if n % 2 == 0 else 2)
    sim.close()


def test_call_captures_into_a_graph():
    """captured once, replayed after the state and udot changed in place, it gives what a direct call gives"""
    n = 65
    st = _states()
    sim = _sim(make_cfg(n, seed=2))
    udot = torch.zeros(n, NG, device="cuda:0")
    out = torch.zeros(n, _nb(sim), 6, device="cuda:0")
    sim.body_accelerations(udot, abi.ACC_ALL, abi.SPACE_LOCAL, out)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        sim.body_accelerations(udot, abi.ACC_ALL, abi.SPACE_LOCAL, out)
    _write_states(sim, st["root"][:n], st["dof"][:n], st["ball"][:n])
    udot.copy_(_dev(st["udot"][:n]).view(n, NG))
    g.replay()
    got = _host(out)
    direct = _call(sim, udot, abi.ACC_ALL, abi.SPACE_LOCAL)
    np.testing.assert_array_equal(_bits(got), _bits(direct))
    assert np.abs(got[:, :, 0:3]).max() > 10
    sim.close()


def test_vec_task_methods():
    """VecTask.accelerometer() for /imu_link equals rows of the ctypes-level call; jacobian_dot_u is the VELOCITY term; body_accelerations
    passes its arguments through"""
    from bez_isaacgym_amd.utils.config import load_config
    from bez_isaacgym_amd.utils.rlgames_utils import get_rlgames_env_creator
    n = 64
    cfg = load_config(["task=bez_kick", "num_envs=%d" % n, "headless=True"])
    env = get_rlgames_env_creator(cfg["task"], "bez_kick", "cuda:0", "cuda:0", 0, True)()
    env.step(torch.rand(n, 18, device=env.device) * 2 - 1)
    nb = _nb(env.sim)
    names = BA.model_of("default")["body_names"]
    assert nb == len(names)
    out = torch.zeros(n, nb, 6, device=env.device)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    udot = torch.rand(n, NG, device=env.device) * 20 - 10
    direct = lambda u, terms, space: env.sim.lib.bez_sim_body_accelerations(env.sim.h, None if u is None else C.c_void_p(u.data_ptr()), terms, space,
                                                                            C.c_void_p(out.data_ptr()), stream)
    for body in ("/imu_link", "/camera", "/left_foot"):
        assert direct(udot, abi.ACC_ALL, abi.SPACE_LOCAL) == 0
        t = env.accelerometer(udot, body) if body != "/imu_link" else env.accelerometer(udot)
        assert tuple(t.shape) == (n, 3) and t.dtype == torch.float32
        np.testing.assert_array_equal(_bits(_host(t)), _bits(_host(out)[:, names.index(body), 0:3]))
    for got, terms, u, space in ((lambda: env.jacobian_dot_u(), abi.ACC_VELOCITY, None, 0), (lambda: env.body_accelerations(udot), abi.ACC_MOTION, udot, 0),
                                 (lambda: env.body_accelerations(udot, abi.ACC_ALL, "local"), abi.ACC_ALL, udot, 1)):
        assert direct(u, terms, space) == 0
        t = got()
        assert tuple(t.shape) == (n, nb, 6) and t.dtype == torch.float32
        np.testing.assert_array_equal(_bits(_host(t)), _bits(_host(out)))
    with pytest.raises(ValueError):
        env.accelerometer(udot, "/no_such_body")
    # standing on the ground after one step: the imu reads about +g along the torso's up axis for udot = 0
    a = _host(env.accelerometer(torch.zeros(n, NG, device=env.device)))
    assert np.isfinite(a).all() and (np.linalg.norm(a, axis=1) > 5).all()
