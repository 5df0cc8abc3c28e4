"""GPU: bez_sim_centroidal (include/bez_sim.h "Centroidal dynamics": centre of mass, momentum about it, the centroidal momentum matrix
A_G, mechanical energy) against the fp64 reference of tests/centroidal_numpy.py, against the mass matrix the library already has, and
against the step itself.

Sizes: 1, 15, 16, 17 (the kernel's 16-env tile), 65 and 300.  No outlier budget anywhere: every element of every env is held to its bar.

  known answer   per block (COM, COM_VEL, LIN_MOM, ANG_MOM, MASS, KINETIC, POTENTIAL, the matrix's linear rows, its angular rows): 3x the
                 worst absolute error of cm_ref evaluated in np.float32 against fp64 on the same states + 2 fp32 ulps of the block's
                 largest |reference|.
  mass matrix    LIN_MOM and ANG_MOM + (COM - root) x LIN_MOM against the refreshed mass_matrix[:, 0:6, :] @ u, KINETIC against
                 1/2 u^T M u, both sides fp32 on the GPU: 1e-5 sum_j sqrt(M_ii M_jj) |u_j| per row + the fp64-evaluated bound of the
                 24-term fp32 dot product, the rule of tests/test_gpu_inverse_dynamics.py for mass_matrix @ udot.
  closure        one substep from 64 states at rest in free space with random position targets: only internal torques act, so the
                 momentum A_G(q0) u1 is the step's own residual; |GPU| <= |fp64 reference on the same read-back| + the known-answer bar.

Measured on MI355X: see DESIGN.md 4.3g."""
import ctypes as C

import numpy as np
import pytest
import torch

from bez_isaacgym_amd import abi
from tests import centroidal_numpy as CM
from tests import dynamics_numpy as D
from tests.centroidal_numpy import centroidal_states
from tests.gpu_util import ASSETS, _bits, _dev, _free, _host, _sim, _write_states
from tests.sim_cfg import make_cfg
from tests.state_sets import ball_states, ulp32

pytestmark = pytest.mark.gpu

TILE = 16
SIZES = (1, TILE - 1, TILE, TILE + 1, 65, 300)
NMAX = max(SIZES)
NG = abi.NUM_GEN
W = abi.CM_WORDS
_CACHE = {}


def _states():
    if "states" not in _CACHE:
        root, dof = centroidal_states(NMAX)
        rng = np.random.default_rng(37)
        scale = rng.uniform(0.5, 1.5, (NMAX, 19)).astype(np.float32)
        gravity = (np.array([0.0, 0.0, -9.81]) + rng.uniform(-2, 2, (NMAX, 3))).astype(np.float32)
        u = np.concatenate([root[:, 7:13], dof[:, :, 1]], axis=1).astype(np.float64)
        _CACHE["states"] = dict(root=root, dof=dof, ball=ball_states(NMAX), scale=scale, gravity=gravity, u=u)
    return _CACHE["states"]


def _bars(r64, r32):
    """{block: 3x the yardstick's worst error + 2 ulps of the block's largest |reference|} for cm_ref results in fp64 and fp32"""
    bars = {}
    for name, sl in CM.STATE_BLOCKS:
        bars[name] = 3.0 * float(np.abs(r32["state"][:, sl].astype(np.float64) - r64["state"][:, sl]).max()) + 2.0 * float(ulp32(np.abs(r64["state"][:, sl]).max()))
    for name, sl in CM.MATRIX_BLOCKS:
        bars[name] = 3.0 * float(np.abs(r32["matrix"][:, sl].astype(np.float64) - r64["matrix"][:, sl]).max()) + 2.0 * float(ulp32(np.abs(r64["matrix"][:, sl]).max()))
    return bars


def _errors(state, matrix, r64):
    """{block: |got - reference| elementwise} over the first len(state) envs"""
    n = state.shape[0]
    out = {name: np.abs(state[:, sl].astype(np.float64) - r64["state"][:n, sl]) for name, sl in CM.STATE_BLOCKS}
    out.update({name: np.abs(matrix[:, sl].astype(np.float64) - r64["matrix"][:n, sl]) for name, sl in CM.MATRIX_BLOCKS})
    return out


def _refs(asset, randomized, cfg):
    """(fp64 reference, bars) of an asset's link model on the NMAX states; computed once per key and left unchanged"""
    key = ("ref", "cleats" if asset == "cleats" else "stl", randomized)
    if key not in _CACHE:
        st = _states()
        g = st["gravity"] if randomized else np.asarray(list(cfg.gravity), np.float64)
        a = (D.model_of(asset), (st["root"], st["dof"]), st["scale"] if randomized else None, g)
        r64 = CM.cm_ref(*a, armature=float(cfg.armature))
        r32 = CM.cm_ref(*a, dtype=np.float32, armature=float(cfg.armature))
        _CACHE[key] = (r64, _bars(r64, r32))
    return _CACHE[key]


def _no_bits(a):
    """+0.0 to the bit"""
    return not _bits(a).any()


def _call(sim, state=True, matrix=True):
    """a raw call into fresh buffers filled with a sentinel -> (state or None, matrix or None) on the host"""
    n = sim.num_envs
    s = torch.full((n, W), -77.0, device="cuda:0") if state else None
    m = torch.full((n, 6, NG), -77.0, device="cuda:0") if matrix else None
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert sim.lib.bez_sim_centroidal(sim.h, ptr(s), ptr(m), stream) == 0, sim.lib.bez_sim_last_error(sim.h)
    return (None if s is None else _host(s)), (None if m is None else _host(m))


def _prepared(cfg, n, randomized):
    st = _states()
    sim = _sim(cfg)
    _write_states(sim, st["root"][:n], st["dof"][:n], st["ball"][:n])
    if randomized:
        sim.set_env_params(abi.PARAM_MASS_SCALE, _dev(st["scale"][:n]))
        sim.set_env_params(abi.PARAM_GRAVITY, _dev(st["gravity"][:n]))
    return sim


@pytest.mark.parametrize("randomized", [False, True], ids=["default_params", "mass_scale_and_gravity_rows"])
@pytest.mark.parametrize("task", ["bez_kick", "bez_walk"])
@pytest.mark.parametrize("asset", list(ASSETS))
def test_known_answer(asset, task, randomized):
    """every word of the state and every element of the matrix against cm_ref in fp64 on the fp32 states, every env, with the default
    parameters and with a random BEZ_PARAM_MASS_SCALE row (0.5 to 1.5 per link) plus a different BEZ_PARAM_GRAVITY row per env"""
    cfg = lambda n: make_cfg(n, task=task, seed=5, **ASSETS[asset])
    r64, bars = _refs(asset, randomized, cfg(1))
    report = {}
    for n in SIZES:
        sim = _prepared(cfg(n), n, randomized)
        state, matrix = _call(sim)
        sim.close()
        assert state.shape == (n, W) and matrix.shape == (n, 6, NG) and state.dtype == matrix.dtype == np.float32
        for name, err in _errors(state, matrix, r64).items():
            report[name] = max(report.get(name, 0.0), float(err.max() / bars[name]))
    print("CM_KNOWN_ANSWER worst error / bar {block}:", asset, task, "randomized" if randomized else "default",
          {k: round(v, 3) for k, v in report.items()}, "bars:", {k: float("%.3g" % v) for k, v in bars.items()})
    assert max(report.values()) <= 1.0, report


@pytest.mark.parametrize("asset", list(ASSETS))
def test_exact_structure(asset):
    """the structural zeros, the mass diagonal, the symmetry of the centroidal inertia and the padding word, to the bit; a state at rest
    has no momentum and no kinetic energy; a zero gravity row leaves no potential energy; each output alone gives the bits of both"""
    st = _states()
    n = 65
    sim = _prepared(make_cfg(n, seed=5, **ASSETS[asset]), n, True)
    state, matrix = _call(sim)
    assert _no_bits(matrix[:, 3:6, 0:3]) and (matrix[:, 3:6, 0:3] == 0.0).all()
    for r in range(3):
        for c in range(3):
            want = state[:, abi.CM_MASS] if r == c else np.zeros(n, np.float32)
            np.testing.assert_array_equal(_bits(matrix[:, r, c]), _bits(want))
    np.testing.assert_array_equal(_bits(matrix[:, 3:6, 3:6]), _bits(np.transpose(matrix[:, 3:6, 3:6], (0, 2, 1))))
    np.testing.assert_array_equal(_bits(state[:, 15]), np.zeros(n, np.uint32))
    assert (matrix[:, [3, 4, 5], [3, 4, 5]] > 0).all() and (state[:, abi.CM_MASS] > 1).all() and np.isfinite(state).all() and np.isfinite(matrix).all()
    # LIN_MOM == MASS * COM_VEL within 1 ulp
    p, v, m = state[:, 6:9].astype(np.float64), state[:, 3:6].astype(np.float64), state[:, abi.CM_MASS].astype(np.float64)[:, None]
    assert (np.abs(p - m * v) <= ulp32(p)).all()
    # each output alone: the same bits, and the other buffer is not an argument
    s_only, none = _call(sim, matrix=False)
    assert none is None
    np.testing.assert_array_equal(_bits(s_only), _bits(state))
    none, m_only = _call(sim, state=False)
    assert none is None
    np.testing.assert_array_equal(_bits(m_only), _bits(matrix))
    # u = 0
    root, dof = st["root"][:n].copy(), st["dof"][:n].copy()
    root[:, 7:13] = 0; dof[:, :, 1] = 0
    _write_states(sim, root, dof, st["ball"][:n])
    rest, rest_matrix = _call(sim)
    assert _no_bits(rest[:, abi.CM_COM_VEL:abi.CM_ANG_MOM + 3]) and _no_bits(rest[:, abi.CM_KINETIC])
    np.testing.assert_array_equal(_bits(rest_matrix), _bits(matrix))       # A_G is a function of the configuration alone
    np.testing.assert_array_equal(_bits(rest[:, 0:3]), _bits(state[:, 0:3]))
    assert np.abs(rest[:, abi.CM_POTENTIAL]).max() > 1
    # a zero gravity row
    sim.set_env_params(abi.PARAM_GRAVITY, _dev(np.zeros((n, 3), np.float32)))
    assert _no_bits(_call(sim, matrix=False)[0][:, abi.CM_POTENTIAL])
    sim.close()


@pytest.mark.parametrize("asset", list(ASSETS))
def test_momentum_and_energy_against_the_mass_matrix(asset):
    """both sides fp32 on the GPU, with a mass-scale row per env: rows 0:6 of mass_matrix @ u are the momentum about the ROOT origin,
    which the call's words give as [LIN_MOM; ANG_MOM + (COM - root) x LIN_MOM]; 1/2 u^T M u is KINETIC"""
    st = _states()
    worst = {"momentum": 0.0, "kinetic": 0.0}
    for n in SIZES:
        sim = _prepared(make_cfg(n, seed=5, **ASSETS[asset]), n, True)
        Mt = sim.dynamics_tensor("mass_matrix")
        sim.refresh_dynamics_tensors("mass_matrix")
        M = _host(Mt).astype(np.float64)
        state, _ = _call(sim, matrix=False)
        sim.close()
        s = state.astype(np.float64)
        u, au = st["u"][:n], np.abs(st["u"][:n])
        rel = s[:, 0:3] - st["root"][:n, 0:3].astype(np.float64)
        got = np.concatenate([s[:, 6:9], s[:, 9:12] + np.cross(rel, s[:, 6:9])], axis=1)
        want = np.einsum("eij,ej->ei", M[:, 0:6], u)
        tol = 1e-5 * np.einsum("eij,ej->ei", D.scale_of(M)[:, 0:6], au) + NG * 2.0 ** -23 * np.einsum("eij,ej->ei", np.abs(M[:, 0:6]), au)
        ratio = np.abs(got - want) / tol
        worst["momentum"] = max(worst["momentum"], float(ratio.max()))
        assert (ratio <= 1.0).all(), (asset, n, float(ratio.max()), [tuple(x) for x in np.argwhere(ratio > 1)[:5]])
        ke = 0.5 * np.einsum("ei,eij,ej->e", u, M, u)
        ktol = 0.5 * (1e-5 * np.einsum("ei,eij,ej->e", au, D.scale_of(M), au) + 2 * NG * 2.0 ** -23 * np.einsum("ei,eij,ej->e", au, np.abs(M), au))
        kratio = np.abs(s[:, abi.CM_KINETIC] - ke) / ktol
        worst["kinetic"] = max(worst["kinetic"], float(kratio.max()))
        assert (kratio <= 1.0).all(), (asset, n, float(kratio.max()))
    print("CM_VS_MASS_MATRIX worst |difference| / tolerance:", asset, {k: round(v, 4) for k, v in worst.items()})


@pytest.mark.parametrize("kernel", ["ws8q", "ws8", "lane"])
def test_momentum_closes_on_the_step(model, kernel, monkeypatch):
    """64 envs at rest in free space (a zero gravity row, the root a metre up, the ball out of reach), random position targets, one
    substep: only internal torques acted, so the momentum of the post-step velocities u1 on the pre-step configuration, A_G(q0) u1, is
    the step's own residual.  The call's LIN_MOM / ANG_MOM on that state (restored with the setters) stay within the fp64 reference's
    residual on the same read-back + the known-answer bar of those states; no separate threshold."""
    from tests.sim_adapter import SimAdapter
    n = 64
    cfg = abi.default_config(n, seed=3)
    cfg.substeps = 1
    monkeypatch.setenv("BEZ_SIM_KERNEL", kernel)
    sim = SimAdapter(cfg)
    sim.set_env_params(abi.PARAM_GRAVITY, np.zeros((n, 3), np.float32))
    sim.step(np.zeros((n, 18), np.float32))
    rng = np.random.default_rng(41)
    dflt = np.asarray(model["dof_default"], float)
    rs = sim.root_states.reshape(n, 2, 13).copy()
    ds = np.zeros((n, 18, 2), np.float32)
    quat = rng.normal(size=(n, 4))
    rs[:, 0, :] = 0
    rs[:, 0, 0:2] = rng.uniform(-1, 1, (n, 2)); rs[:, 0, 2] = rng.uniform(1.0, 1.5, n)
    rs[:, 0, 3:7] = quat / np.linalg.norm(quat, axis=1, keepdims=True)
    rs[:, 1, :] = 0; rs[:, 1, 0:3] = (0.0, 4.0, 0.08); rs[:, 1, 6] = 1.0
    ds[:, :, 0] = dflt[None] + rng.uniform(-0.05, 0.05, (n, 18))
    acts = (ds[:, :, 0] + rng.uniform(-0.5, 0.5, (n, 18)) - dflt[None]).astype(np.float32)
    sim.set_root_states(rs.reshape(-1, 13)); sim.set_dof_state(ds.reshape(-1, 2))
    rs0, ds0 = sim.root_states.reshape(n, 2, 13).copy(), sim.dof_state.reshape(n, 18, 2).copy()
    sim.pre_physics(acts); sim.simulate()
    rs1, ds1 = sim.root_states.reshape(n, 2, 13).copy(), sim.dof_state.reshape(n, 18, 2).copy()
    back_r, back_d = rs0.copy(), ds0.copy()
    back_r[:, 0, 7:13] = rs1[:, 0, 7:13]; back_d[:, :, 1] = ds1[:, :, 1]
    sim.set_root_states(back_r.reshape(-1, 13)); sim.set_dof_state(back_d.reshape(-1, 2))
    np.testing.assert_array_equal(sim.dof_state.reshape(n, 18, 2), back_d)
    state, matrix = _call(sim.sim)
    a = (D.model_of("default"), (back_r[:, 0], back_d), None, np.zeros(3))
    r64 = CM.cm_ref(*a, armature=float(cfg.armature))
    bars = _bars(r64, CM.cm_ref(*a, dtype=np.float32, armature=float(cfg.armature)))
    u1 = np.concatenate([back_r[:, 0, 7:13], back_d[:, :, 1]], axis=1).astype(np.float64)
    gross = np.einsum("eij,ej->ei", np.abs(r64["matrix"]), np.abs(u1))
    res = {}
    for name, sl in (("lin_mom", slice(6, 9)), ("ang_mom", slice(9, 12))):
        got, ref = np.abs(state[:, sl].astype(np.float64)), np.abs(r64["state"][:, sl])
        res[name] = (float(got.max()), float(ref.max()), bars[name])
        assert (got <= ref + bars[name]).all(), (name, float((got - ref).max()), bars[name])
    print("CM_CLOSURE kernel=%s worst |LIN_MOM| %.3g (fp64 on the same read-back %.3g, bar %.3g) kg m/s, |ANG_MOM| %.3g (fp64 %.3g, bar %.3g) kg m^2/s; "
          "gross momentum sum_j |A_G[:, j] u_j|: linear %.3g, angular %.3g; largest |u1| %.3g"
          % ((kernel,) + res["lin_mom"] + res["ang_mom"] + (float(gross[:, 0:3].max()), float(gross[:, 3:6].max()), float(np.abs(u1).max()))))
    assert np.abs(u1[:, 6:]).max() > 1.0 and gross[:, 0:3].max() > 1e-2 and gross[:, 3:6].max() > 1e-3   # not vacuous: the drives moved the joints


def test_contract():
    """both pointers null: rc -1 with a message that names the function (for a null sim too); ten calls allocate nothing; the sim's state is
    untouched; a side stream and views that are only 4-byte aligned give the direct call's bits; the Python layer checks what it is handed"""
    from bez_isaacgym_amd.sim import BezSimError
    n = 65
    sim = _prepared(make_cfg(n, seed=2), n, False)
    state, matrix = torch.zeros(n, W, device="cuda:0"), torch.zeros(n, 6, NG, device="cuda:0")
    torch.cuda.synchronize()
    assert sim.lib.bez_sim_centroidal(sim.h, None, None, None) == -1
    assert b"bez_sim_centroidal" in sim.lib.bez_sim_last_error(sim.h)
    assert sim.lib.bez_sim_centroidal(None, C.c_void_p(state.data_ptr()), C.c_void_p(matrix.data_ptr()), None) == -1
    assert b"bez_sim_centroidal" in sim.lib.bez_sim_last_error(None)
    assert not state.any() and not matrix.any()
    # every tensor the sim keeps or derives from its state, the per-env parameters included
    everything = (abi.TENSOR_ROOT_STATE, abi.TENSOR_DOF_STATE, abi.TENSOR_RIGID_BODY_STATE, abi.TENSOR_NET_CONTACT_FORCE, abi.TENSOR_OBS, abi.TENSOR_REW,
                  abi.TENSOR_RESET, abi.TENSOR_PROGRESS, abi.TENSOR_DOF_TARGET, abi.TENSOR_PREV_LIN_VEL, abi.TENSOR_FEET, abi.TENSOR_GOAL)
    snap = lambda: [_host(sim.refresh(w)) for w in everything] + [_host(sim.get_env_params(p)) for p in (abi.PARAM_MASS_SCALE, abi.PARAM_GRAVITY)]
    before_state = snap()
    want_s, want_m = _call(sim)
    sim.centroidal(want_matrix=True)       # the sim's own result buffers exist from here on
    before = _free()
    for k in range(10):
        sim.centroidal(state if k % 2 else None, matrix if k % 3 else None, want_matrix=bool(k % 4))
    assert _free() == before
    for a, b in zip(before_state, snap()):
        np.testing.assert_array_equal(a.view(np.uint8), b.view(np.uint8))
    s, m = sim.centroidal(state, matrix)
    assert s is state and m is matrix
    np.testing.assert_array_equal(_bits(_host(state)), _bits(want_s))
    np.testing.assert_array_equal(_bits(_host(matrix)), _bits(want_m))
    assert sim.centroidal(state)[1] is None
    state.zero_(); matrix.zero_()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        sim.centroidal(state, matrix)
    np.testing.assert_array_equal(_bits(_host(state)), _bits(want_s))
    np.testing.assert_array_equal(_bits(_host(matrix)), _bits(want_m))
    assert np.abs(want_s[:, 6:9]).max() > 1
    # views that are contiguous but only 4-byte aligned take the kernel's scalar path: same bits, nothing outside them written
    pad_s, pad_m = torch.full((n * W + 2,), 5.0, device="cuda:0"), torch.full((n * 6 * NG + 2,), 5.0, device="cuda:0")
    sim.centroidal(pad_s[1:-1].view(n, W), pad_m[1:-1].view(n, 6, NG))
    np.testing.assert_array_equal(_bits(_host(pad_s[1:-1].view(n, W))), _bits(want_s))
    np.testing.assert_array_equal(_bits(_host(pad_m[1:-1].view(n, 6, NG))), _bits(want_m))
    assert _host(pad_s)[[0, -1]].tolist() == [5.0, 5.0] and _host(pad_m)[[0, -1]].tolist() == [5.0, 5.0]
    # one aligned, one not
    sim.centroidal(state.zero_(), pad_m[1:-1].view(n, 6, NG))
    np.testing.assert_array_equal(_bits(_host(state)), _bits(want_s))
    for bad in (dict(state=state[:, :15]), dict(state=state.double()), dict(state=state.cpu()), dict(state=state.t().contiguous().t()),
                dict(state=state.reshape(-1)), dict(state=_host(state)), dict(matrix=matrix[:-1]), dict(matrix=matrix.reshape(n, 6 * NG)),
                dict(matrix=matrix.double()), dict(matrix=matrix.cpu()), dict(matrix=matrix.transpose(1, 2).contiguous().transpose(1, 2))):
        with pytest.raises(BezSimError):
            sim.centroidal(**bad)
    sim.close()


def test_call_captures_into_a_graph():
    """captured once, replayed after the state changed in place, it gives what a direct call gives"""
    n = 65
    st = _states()
    sim = _sim(make_cfg(n, seed=2))
    state, matrix = torch.zeros(n, W, device="cuda:0"), torch.zeros(n, 6, NG, device="cuda:0")
    sim.centroidal(state, matrix)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        sim.centroidal(state, matrix)
    _write_states(sim, st["root"][:n], st["dof"][:n], st["ball"][:n])
    g.replay()
    got_s, got_m = _host(state), _host(matrix)
    want_s, want_m = _call(sim)
    np.testing.assert_array_equal(_bits(got_s), _bits(want_s))
    np.testing.assert_array_equal(_bits(got_m), _bits(want_m))
    assert np.abs(got_s[:, 6:9]).max() > 1
    sim.close()


def test_vec_task_methods():
    """the VecTask wrappers return views of one call's output, equal to the ctypes-level call's bits"""
    from bez_isaacgym_amd.utils.config import load_config
    from bez_isaacgym_amd.utils.rlgames_utils import get_rlgames_env_creator
    n = 64
    cfg = load_config(["task=bez_kick", "num_envs=%d" % n, "headless=True"])
    env = get_rlgames_env_creator(cfg["task"], "bez_kick", "cuda:0", "cuda:0", 0, True)()
    env.step(torch.rand(n, 18, device=env.device) * 2 - 1)
    want_s, want_m = _call(env.sim)
    s = env.centroidal_state()
    assert tuple(s.shape) == (n, W) and s.dtype == torch.float32
    np.testing.assert_array_equal(_bits(_host(s)), _bits(want_s))
    pos, vel = env.center_of_mass()
    ke, pe = env.mechanical_energy()
    mom = env.centroidal_momentum()
    A = env.centroidal_momentum_matrix()
    for view, first, shape in ((pos, abi.CM_COM, (n, 3)), (vel, abi.CM_COM_VEL, (n, 3)), (mom, abi.CM_LIN_MOM, (n, 6)), (ke, abi.CM_KINETIC, (n,)),
                               (pe, abi.CM_POTENTIAL, (n,))):
        assert tuple(view.shape) == shape and view.data_ptr() == s.data_ptr() + 4 * first
        np.testing.assert_array_equal(_bits(_host(view)), _bits(want_s[:, first:first + (shape[1] if len(shape) > 1 else 1)].reshape(shape)))
    assert tuple(A.shape) == (n, 6, NG)
    np.testing.assert_array_equal(_bits(_host(A)), _bits(want_m))
    h = _host(s)
    assert np.isfinite(h).all() and (h[:, abi.CM_MASS] > 1).all() and (h[:, abi.CM_POTENTIAL] > 1).all()   # the robot stands above z = 0 under -g
