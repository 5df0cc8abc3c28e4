"""GPU: bez_sim_forward_dynamics (include/bez_sim.h "Forward dynamics": udot = M^-1 (f - h), rows [root_lin; root_ang; qdd]) against the
fp64 reference of tests/forward_dynamics_numpy.py, against bez_sim_inverse_dynamics on the GPU, and against its own contract.

Sizes: 1, 65, 300 and, around the kernel's 16-env tile, 15, 16, 17.  Forces: +-5 N on rows 0:3, +-0.5 N m on the others.  No outlier
budget anywhere: every element of every env is held to its bar.

  known answer   per block (rows 0:3, 3:6, 6:24), bias set and base mode: 3x the worst absolute error of fd_ref_batch evaluated in
                 np.float32 against fp64 on the same states + 2 fp32 ulps of the block's largest |reference|.
  round trip     inverse_dynamics(forward_dynamics(f, bias), ID_INERTIA | bias) against f, both fp32 on the GPU.  Per row the bar of
                 test_inertia_term_is_the_mass_matrix_times_udot at the returned udot with M from the refreshed tensor,
                 1e-5 sum_j sqrt(M_ii M_jj) |udot_j| + 24 * 2^-23 * sum_j |M_ij| |udot_j|, plus 3x the residual of the same round trip of
                 the references evaluated in np.float32 on those states (per block, the worst over the envs: one element's residual is a
                 sample of a rounding error, the block's worst is its size).

Measured on MI355X: known answer, worst error / bar over the 12 cases 0.91 (cleats, bias 0, floating base, rows 3:6),
joint rows 0.81; round trip 0.041 of its bar, 0.042 of the mass-matrix part alone (the references' residual adds 7e-6 N m to a joint
row's bar); free fall 0.82."""
import ctypes as C

import numpy as np
import pytest
import torch

from bez_isaacgym_amd import abi
from tests import dynamics_numpy as D
from tests import forward_dynamics_numpy as FD
from tests import inverse_dynamics_numpy as ID
from tests.gpu_util import ASSETS, _bits, _dev, _free, _host, _prepared, _sim, _states, _write_states
from tests.sim_cfg import make_cfg
from tests.state_sets import ulp32

pytestmark = pytest.mark.gpu

TILE = 16
SIZES = (1, TILE - 1, TILE, TILE + 1, 65, 300)
NMAX = max(SIZES)
NG = abi.NUM_GEN
BIAS_ALL = abi.ID_VELOCITY | abi.ID_GRAVITY
BIASES = (BIAS_ALL, abi.ID_VELOCITY, abi.ID_GRAVITY, 0)
LEFT_LEG = FD.CHAINS[2]
_CACHE = {}


def _forces():
    if "forces" not in _CACHE:
        rng = np.random.default_rng(41)
        _CACHE["forces"] = (rng.uniform(-1, 1, (NMAX, NG)) * np.where(np.arange(NG) < 3, 5.0, 0.5)).astype(np.float32)
    return _CACHE["forces"]


def _model_args(asset, randomized, cfg):
    st = _states()
    g = st["gravity"] if randomized else np.asarray(list(cfg.gravity), np.float64)
    return D.model_of(asset), st["root"], st["dof"], _forces(), g, (st["scale"] if randomized else None), float(cfg.armature)


def _block_bar(r32, r64):
    bar = np.zeros(NG)
    for _, sl in FD.BLOCKS:
        bar[sl] = 3.0 * float(np.abs(r32[:, sl] - r64[:, sl]).max()) + 2.0 * float(ulp32(np.abs(r64[:, sl]).max()))
    return bar


def _refs(asset, randomized, cfg):
    """{(bias, fixed): (fp64 reference (NMAX, 24), bar (24,), round-trip residual of the fp32 references per block (24,))} of an asset's
    link model; computed once per key and left unchanged"""
    key = ("ref", "cleats" if asset == "cleats" else "stl", randomized)
    if key not in _CACHE:
        a = _model_args(asset, randomized, cfg)
        model, root, dof, force, g, scale, arm = a
        M = {f: FD.M_batch(model, root, dof, scale, arm, f) for f in (np.float64, np.float32)}
        out = {}
        for bias in BIASES:
            for fixed in (False, True):
                r64 = FD.fd_ref_batch(*a, bias, fixed, M=M[np.float64])
                r32 = FD.fd_ref_batch(*a, bias, fixed, dtype=np.float32, M=M[np.float32])
                back = ID.id_ref_batch(model, root, dof, r32, g, scale, arm, abi.ID_INERTIA | bias, dtype=np.float32)
                resid = np.zeros(NG)
                for _, sl in FD.BLOCKS:
                    resid[sl] = float(np.abs(back[:, sl].astype(np.float64) - force[:, sl]).max())
                out[bias, fixed] = (r64, _block_bar(r32.astype(np.float64), r64), resid)
        _CACHE[key] = out
    return _CACHE[key]


def _fd_sim(cfg, n, randomized):
    sim, _ = _prepared(cfg, n, randomized)
    return sim, _dev(_forces()[:n]).view(n, NG)


def _call(sim, force, bias=BIAS_ALL, fixed=False, out=None):
    return _host(sim.forward_dynamics(force, bias, fixed, out))


def _rows(fixed):
    return [(name, sl) for name, sl in FD.BLOCKS if not (fixed and sl.stop <= 6)]


@pytest.mark.parametrize("randomized", [False, True], ids=["default_params", "mass_scale_and_gravity_rows"])
@pytest.mark.parametrize("task", ["bez_kick", "bez_walk"])
@pytest.mark.parametrize("asset", list(ASSETS))
def test_known_answer(asset, task, randomized):
    """every bias set, floating and fixed base, against fd_ref_batch in fp64 on the fp32 states, every element of every env, with the
    default parameters and with a random BEZ_PARAM_MASS_SCALE row (0.5 to 1.5 per link) plus a different BEZ_PARAM_GRAVITY row per env"""
    cfg = lambda n: make_cfg(n, task=task, seed=5, **ASSETS[asset])
    refs = _refs(asset, randomized, cfg(1))
    report = {}
    for n in SIZES:
        sim, force = _fd_sim(cfg(n), n, randomized)
        for (bias, fixed), (ref, bar, _) in refs.items():
            got = _call(sim, force, bias, fixed)
            assert got.shape == (n, NG) and got.dtype == np.float32
            err = np.abs(got.astype(np.float64) - ref[:n])
            for name, sl in _rows(fixed):
                report[bias, fixed, name] = max(report.get((bias, fixed, name), 0.0), float((err[:, sl] / bar[sl]).max()))
            if fixed:
                assert not _bits(got[:, 0:6]).any()
        sim.close()
    print("FD_KNOWN_ANSWER worst error / bar {(bias, fixed base, block)}:", asset, task, "randomized" if randomized else "default",
          {k: round(v, 3) for k, v in report.items()}, "bars (all bias, floating):", [float(refs[BIAS_ALL, False][1][sl][0]) for _, sl in FD.BLOCKS])
    assert max(report.values()) <= 1.0, report


@pytest.mark.parametrize("asset", list(ASSETS))
def test_round_trip_through_inverse_dynamics(asset):
    """both calls fp32 on the GPU, with a mass-scale and a gravity row per env"""
    worst, worst_own = 0.0, 0.0
    f64 = _forces().astype(np.float64)
    for n in (TILE + 1, NMAX):
        cfg = make_cfg(n, seed=5, **ASSETS[asset])
        refs = _refs(asset, True, cfg)
        sim, force = _fd_sim(cfg, n, True)
        Mt = sim.dynamics_tensor("mass_matrix")
        sim.refresh_dynamics_tensors("mass_matrix")
        M = _host(Mt).astype(np.float64)
        for (bias, fixed), (_, _, resid) in refs.items():
            udot = sim.forward_dynamics(force, bias, fixed)
            x = np.abs(_host(udot).astype(np.float64))
            back = _host(sim.inverse_dynamics(udot, abi.ID_INERTIA | bias)).astype(np.float64)
            own = 1e-5 * np.einsum("eij,ej->ei", D.scale_of(M), x) + NG * 2.0 ** -23 * np.einsum("eij,ej->ei", np.abs(M), x)
            lo = 6 if fixed else 0
            err = np.abs(back - f64[:n])[:, lo:]
            ratio = err / (own + 3.0 * resid[None, :])[:, lo:]
            worst, worst_own = max(worst, float(ratio.max())), max(worst_own, float((err / own[:, lo:]).max()))
            assert (ratio <= 1.0).all(), (asset, n, bias, fixed, float(ratio.max()), [tuple(i) for i in np.argwhere(ratio > 1)[:5]])
        sim.close()
    print("FD_ROUND_TRIP worst |ID(FD(f)) - f| / bar:", asset, round(worst, 3), "against the mass-matrix part of the bar alone:", round(worst_own, 3),
          "reference residual per block (all bias, floating):", [float(refs[BIAS_ALL, False][2][sl][0]) for _, sl in FD.BLOCKS])


@pytest.mark.parametrize("asset", list(ASSETS))
def test_free_fall(asset):
    """u = 0, no force, the gravity term, a floating base: every link falls with g -- udot = [g, 0 x 21] with g the env's own row --
    within the known-answer bar of these states"""
    n = 65
    st = _states()
    cfg = make_cfg(n, seed=5, **ASSETS[asset])
    sim = _sim(cfg)
    root, dof = st["root"][:n].copy(), st["dof"][:n].copy()
    root[:, 7:13] = 0; dof[:, :, 1] = 0
    _write_states(sim, root, dof, st["ball"][:n])
    sim.set_env_params(abi.PARAM_MASS_SCALE, _dev(st["scale"][:n]))
    sim.set_env_params(abi.PARAM_GRAVITY, _dev(st["gravity"][:n]))
    got = _call(sim, None, abi.ID_GRAVITY).astype(np.float64)
    sim.close()
    a = (D.model_of(asset), root, dof, None, st["gravity"][:n], st["scale"][:n], float(cfg.armature), abi.ID_GRAVITY, False)
    r64 = FD.fd_ref_batch(*a)
    bar = _block_bar(FD.fd_ref_batch(*a, dtype=np.float32).astype(np.float64), r64)
    want = np.concatenate([st["gravity"][:n].astype(np.float64), np.zeros((n, NG - 3))], axis=1)
    # (printed, not asserted: the fp32 quaternions are unit to 6e-8 and the reference's M and h take them as they are, each in its own
    # way, so the reference itself is [g, 0] only to about 2e-5 here; the call is held to [g, 0])
    ref_ratio = np.abs(r64 - want) / bar
    ratio = np.abs(got - want) / bar
    print("FD_FREE_FALL worst error / bar per block:", asset, [round(float(ratio[:, sl].max()), 3) for _, sl in FD.BLOCKS], "bars:",
          [float(bar[sl][0]) for _, sl in FD.BLOCKS], "the fp64 reference against [g, 0]:", round(float(ref_ratio.max()), 4))
    assert (ratio <= 1.0).all(), float(ratio.max())


@pytest.mark.parametrize("asset", list(ASSETS))
def test_exact_structure(asset):
    """fixed base: rows 0:6 are +0.0f; with bias 0 a chain without force returns +0.0f and a chain's rows do not depend on the others';
    rows 0:6 of the force take no part; `out` may be `force`"""
    n = 65
    sim, force = _fd_sim(make_cfg(n, seed=5, **ASSETS[asset]), n, False)
    full = _call(sim, force, 0, True)
    assert not _bits(full[:, 0:6]).any() and np.abs(full[:, 6:]).min() > 0
    assert not _bits(_call(sim, force, BIAS_ALL, True)[:, 0:6]).any()
    leg = torch.zeros_like(force)
    leg[:, LEFT_LEG] = force[:, LEFT_LEG]
    got = _call(sim, leg, 0, True)
    other = np.ones(NG, bool); other[LEFT_LEG] = False
    assert not _bits(got[:, other]).any()
    np.testing.assert_array_equal(_bits(got[:, LEFT_LEG]), _bits(full[:, LEFT_LEG]))
    poisoned = force.clone()
    poisoned[:, 0:6] = float("nan")
    np.testing.assert_array_equal(_bits(_call(sim, poisoned, BIAS_ALL, True)), _bits(_call(sim, force, BIAS_ALL, True)))
    for bias, fixed in ((BIAS_ALL, False), (0, False), (abi.ID_GRAVITY, True)):
        want = _call(sim, force, bias, fixed)
        buf = force.clone()
        assert sim.forward_dynamics(buf, bias, fixed, buf) is buf
        np.testing.assert_array_equal(_bits(_host(buf)), _bits(want))
    sim.close()


def test_bits_do_not_depend_on_the_number_of_envs():
    """env e of the N = 300 run has the bits of env e of every smaller run, in every mode"""
    cfg = lambda n: make_cfg(n, seed=5)
    modes = ((BIAS_ALL, False), (0, False), (BIAS_ALL, True))
    sim, force = _fd_sim(cfg(NMAX), NMAX, True)
    big = [_call(sim, force, b, f) for b, f in modes]
    sim.close()
    for n in SIZES[:-1]:
        sim, force = _fd_sim(cfg(n), n, True)
        for (b, f), want in zip(modes, big):
            np.testing.assert_array_equal(_bits(_call(sim, force, b, f)), _bits(want[:n]))
        sim.close()


def test_a_nan_stays_in_its_env():
    """N = 17: a NaN in one env's q, and in another run a NaN in its force row -- every other env has the bits of the clean run and the
    poisoned env's output is not finite"""
    n, bad = TILE + 1, 5
    st = _states()
    sim, force = _fd_sim(make_cfg(n, seed=5), n, True)
    modes = ((BIAS_ALL, False), (BIAS_ALL, True))
    clean = [_call(sim, force, b, f) for b, f in modes]
    assert all(np.isfinite(c).all() for c in clean)
    keep = np.arange(n) != bad
    f_nan = force.clone()
    f_nan[bad, 9] = float("nan")
    for (b, f), want in zip(modes, clean):
        got = _call(sim, f_nan, b, f)
        np.testing.assert_array_equal(_bits(got[keep]), _bits(want[keep]))
        assert not np.isfinite(got[bad]).all()
    dof = st["dof"][:n].copy()
    dof[bad, 7, 0] = np.nan
    _write_states(sim, st["root"][:n], dof, st["ball"][:n])
    for (b, f), want in zip(modes, clean):
        got = _call(sim, force, b, f)
        np.testing.assert_array_equal(_bits(got[keep]), _bits(want[keep]))
        assert not np.isfinite(got[bad]).all()
    sim.close()


def test_contract():
    """bad bias, mode or pointers: rc -1 with a message that names the function, nothing written; ten calls allocate nothing; the sim's
    state is untouched; a side stream and 4-byte-aligned views give the same bits; the Python layer checks what it is handed"""
    from bez_isaacgym_amd.sim import BezSimError
    n = 65
    sim, force = _fd_sim(make_cfg(n, seed=2), n, False)
    out = torch.zeros(n, NG, device="cuda:0")
    torch.cuda.synchronize()
    fptr, optr = C.c_void_p(force.data_ptr()), C.c_void_p(out.data_ptr())
    raw = lambda f, bias, mode, o: sim.lib.bez_sim_forward_dynamics(sim.h, f, bias, mode, o, None)
    for args in ((fptr, abi.ID_INERTIA, 0, optr), (fptr, abi.ID_ALL, 0, optr), (fptr, 8, 0, optr), (fptr, 1 << 31, 0, optr), (None, 0, 0, optr),
                 (None, 0, abi.FD_FIXED_BASE, optr), (fptr, BIAS_ALL, 2, optr), (fptr, BIAS_ALL, 3, optr), (fptr, BIAS_ALL, 0, None)):
        assert raw(*args) == -1, args[1:3]
        assert b"bez_sim_forward_dynamics" in sim.lib.bez_sim_last_error(sim.h)
    assert not out.any()
    snap = lambda: [_host(sim.refresh(w)) for w in (abi.TENSOR_ROOT_STATE, abi.TENSOR_DOF_STATE, abi.TENSOR_DOF_TARGET)]
    state = snap()
    want = _call(sim, force)
    before = _free()
    for k in range(10):
        sim.forward_dynamics(force if k % 2 else None, BIASES[k % 3], bool(k % 4 == 0), out if k % 3 else None)
    assert _free() == before
    for a, b in zip(state, snap()):
        np.testing.assert_array_equal(_bits(a), _bits(b))
    assert raw(fptr, BIAS_ALL, 0, optr) == 0
    np.testing.assert_array_equal(_bits(_host(out)), _bits(want))
    out.zero_()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        sim.forward_dynamics(force, BIAS_ALL, False, out)
    np.testing.assert_array_equal(_bits(_host(out)), _bits(want))
    assert np.abs(want).max() > 1
    # views that are contiguous but only 4-byte aligned take the kernel's scalar path: same bits
    pad_f, pad_o = torch.zeros(n * NG + 1, device="cuda:0"), torch.zeros(n * NG + 1, device="cuda:0")
    pad_f[1:] = force.reshape(-1)
    sim.forward_dynamics(pad_f[1:].view(n, NG), BIAS_ALL, False, pad_o[1:].view(n, NG))
    np.testing.assert_array_equal(_bits(_host(pad_o[1:].view(n, NG))), _bits(want))
    for bad in (dict(force=force[:, :23]), dict(force=force.double()), dict(force=force.cpu()), dict(force=force.t().contiguous().t()), dict(out=out[:-1]),
                dict(out=out.reshape(-1)), dict(force=_host(force)), dict(bias=abi.ID_INERTIA), dict(bias=16), dict(bias=0), dict(force=force, bias=abi.ID_ALL)):
        with pytest.raises(BezSimError):
            sim.forward_dynamics(**bad)
    sim.close()


def test_call_captures_into_a_graph():
    """captured once, replayed after the state and the force changed in place, it gives what a direct call gives"""
    n = 65
    st = _states()
    sim = _sim(make_cfg(n, seed=2))
    force = torch.zeros(n, NG, device="cuda:0")
    out = torch.zeros(n, NG, device="cuda:0")
    sim.forward_dynamics(force, BIAS_ALL, False, out)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        sim.forward_dynamics(force, BIAS_ALL, False, out)
    _write_states(sim, st["root"][:n], st["dof"][:n], st["ball"][:n])
    force.copy_(_dev(_forces()[:n]).view(n, NG))
    g.replay()
    got = _host(out)
    direct = _call(sim, force)
    np.testing.assert_array_equal(_bits(got), _bits(direct))
    assert np.abs(got[:, 0:3]).max() > 1
    sim.close()


def test_vec_task_methods():
    """VecTask.forward_dynamics, free_acceleration and mass_solve equal the ctypes-level call; free_acceleration of a stepped kick env
    is finite"""
    from bez_isaacgym_amd.utils.config import load_config
    from bez_isaacgym_amd.utils.rlgames_utils import get_rlgames_env_creator
    n = 64
    cfg = load_config(["task=bez_kick", "num_envs=%d" % n, "headless=True"])
    env = get_rlgames_env_creator(cfg["task"], "bez_kick", "cuda:0", "cuda:0", 0, True)()
    env.step(torch.rand(n, 18, device=env.device) * 2 - 1)
    out = torch.zeros(n, NG, device=env.device)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    f = torch.rand(n, NG, device=env.device) - 0.5
    fixed = bool(int(env.sim.cfg.flags) & abi.FLAG_FIX_BASE)
    assert not fixed
    for got, bias, mode, force in ((lambda: env.free_acceleration(), BIAS_ALL, 0, None), (lambda: env.mass_solve(f), 0, 0, f),
                                   (lambda: env.forward_dynamics(f), BIAS_ALL, 0, f), (lambda: env.forward_dynamics(f, abi.ID_GRAVITY, True), abi.ID_GRAVITY, 1, f)):
        assert env.sim.lib.bez_sim_forward_dynamics(env.sim.h, None if force is None else C.c_void_p(force.data_ptr()), bias, mode, C.c_void_p(out.data_ptr()), stream) == 0
        t = got()
        assert tuple(t.shape) == (n, NG) and t.dtype == torch.float32
        np.testing.assert_array_equal(_bits(_host(t)), _bits(_host(out)))
    a = _host(env.free_acceleration())
    assert np.isfinite(a).all() and np.abs(a).max() > 1
