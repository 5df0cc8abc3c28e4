"""GPU: bez_sim_inverse_dynamics (include/bez_sim.h "Inverse dynamics": M(q) udot + h(q, u), rows [force; moment about the root origin;
joint torques]) against the fp64 reference of tests/inverse_dynamics_numpy.py, against the mass matrix, and against the step itself.

Sizes: 1, 63, 64, 65, 300 and, around the kernel's 16-env tile, 15, 16, 17.  No outlier budget anywhere: every element of every env is
held to its bar.

  known answer   per block (rows 0:3, 3:6, 6:24): 3x the worst absolute error of id_ref evaluated in np.float32 against fp64 on the same
                 states + 2 fp32 ulps of the block's largest |reference|.
  M udot         inverse_dynamics(udot, ID_INERTIA) against the refreshed mass matrix times udot, both fp32 on the GPU:
                 1e-5 sum_j sqrt(M_ii M_jj) |udot_j| per row (DESIGN.md 4.3e measured M at 3.9e-6 of sqrt(M_ii M_jj); this kernel rounds
                 the same sums) + the fp64-evaluated bound of the 24-term fp32 dot product, 24 * 2^-23 * sum_j |M_ij| |udot_j|.
  closure        one substep from 64 pressed states in free space: M udot + h on the pre-step state, udot = (u1 - u0) / h, equals
                 [0 x 6; DOF_FORCE] within 2e-2 N / N m, the bar tests/test_gpu_dof_force.py uses for the same identity.

Measured on MI355X: see DESIGN.md 4.3f."""
import ctypes as C

import numpy as np
import pytest
import torch

from bez_isaacgym_amd import abi
from tests import dof_force_numpy as DF
from tests import dynamics_numpy as D
from tests import inverse_dynamics_numpy as ID
from tests.gpu_util import ASSETS, _bits, _dev, _free, _host, _prepared, _sim, _states, _write_states
from tests.sim_cfg import make_cfg
from tests.state_sets import ulp32

pytestmark = pytest.mark.gpu

TILE = 16
SIZES = (1, TILE - 1, TILE, TILE + 1, 63, 64, 65, 300)
NMAX = max(SIZES)
NG = abi.NUM_GEN
TERMS = (abi.ID_ALL, abi.ID_INERTIA, abi.ID_VELOCITY, abi.ID_GRAVITY)
_CACHE = {}


def _refs(asset, randomized, cfg):
    """{terms: (fp64 reference (NMAX, 24), bar (24,))} of an asset's link model; computed once per key and left unchanged"""
    key = ("ref", "cleats" if asset == "cleats" else "stl", randomized)
    if key not in _CACHE:
        st = _states()
        g = st["gravity"] if randomized else np.asarray(list(cfg.gravity), np.float64)
        scale = st["scale"] if randomized else None
        out = {}
        for terms in TERMS:
            a = (D.model_of(asset), st["root"], st["dof"], st["udot"], g, scale, float(cfg.armature), terms)
            r64 = ID.id_ref_batch(*a)
            r32 = ID.id_ref_batch(*a, dtype=np.float32).astype(np.float64)
            bar = np.zeros(NG)
            for _, sl in ID.BLOCKS:
                bar[sl] = 3.0 * float(np.abs(r32[:, sl] - r64[:, sl]).max()) + 2.0 * float(ulp32(np.abs(r64[:, sl]).max()))
            out[terms] = (r64, bar)
        _CACHE[key] = out
    return _CACHE[key]


def _call(sim, udot, terms):
    return _host(sim.inverse_dynamics(udot, terms))


@pytest.mark.parametrize("randomized", [False, True], ids=["default_params", "mass_scale_and_gravity_rows"])
@pytest.mark.parametrize("task", ["bez_kick", "bez_walk"])
@pytest.mark.parametrize("asset", list(ASSETS))
def test_known_answer(asset, task, randomized):
    """all three terms together and each term alone against id_ref in fp64 on the fp32 states, every element of every env, with the
    default parameters and with a random BEZ_PARAM_MASS_SCALE row (0.5 to 1.5 per link) plus a different BEZ_PARAM_GRAVITY row per env"""
    cfg = lambda n: make_cfg(n, task=task, seed=5, **ASSETS[asset])
    refs = _refs(asset, randomized, cfg(1))
    report = {}
    for n in SIZES:
        sim, udot = _prepared(cfg(n), n, randomized)
        for terms in TERMS:
            ref, bar = refs[terms]
            got = _call(sim, udot, terms)
            assert got.shape == (n, NG) and got.dtype == np.float32
            err = np.abs(got.astype(np.float64) - ref[:n])
            for name, sl in ID.BLOCKS:
                report[terms, name] = max(report.get((terms, name), 0.0), float((err[:, sl] / bar[sl]).max()))
        sim.close()
    print("ID_KNOWN_ANSWER worst error / bar {(terms, block)}:", asset, task, "randomized" if randomized else "default",
          {k: round(v, 3) for k, v in report.items()}, "bars (all terms):", [float(refs[abi.ID_ALL][1][sl][0]) for _, sl in ID.BLOCKS])
    assert max(report.values()) <= 1.0, report


@pytest.mark.parametrize("asset", list(ASSETS))
def test_inertia_term_is_the_mass_matrix_times_udot(asset):
    """both sides fp32 on the GPU, with a mass-scale row per env"""
    st = _states()
    worst = 0.0
    for n in SIZES:
        sim, udot = _prepared(make_cfg(n, seed=5, **ASSETS[asset]), n, True)
        Mt = sim.dynamics_tensor("mass_matrix")
        sim.refresh_dynamics_tensors("mass_matrix")
        M = _host(Mt).astype(np.float64)
        got = _call(sim, udot, abi.ID_INERTIA).astype(np.float64)
        sim.close()
        ud = np.abs(st["udot"][:n].astype(np.float64))
        want = np.einsum("eij,ej->ei", M, st["udot"][:n].astype(np.float64))
        tol = 1e-5 * np.einsum("eij,ej->ei", D.scale_of(M), ud) + NG * 2.0 ** -23 * np.einsum("eij,ej->ei", np.abs(M), ud)
        ratio = np.abs(got - want) / tol
        worst = max(worst, float(ratio.max()))
        assert (ratio <= 1.0).all(), (asset, n, float(ratio.max()), [tuple(x) for x in np.argwhere(ratio > 1)[:5]])
    print("ID_VS_MASS_MATRIX worst |ID - M udot| / tolerance:", asset, round(worst, 3))


@pytest.mark.parametrize("kernel", ["ws8q", "ws8", "lane"])
def test_equation_of_motion_closes_on_the_step(model, kernel, monkeypatch):
    """64 pressed states in free space (gravity off, hip rolls apart and no leg <-> leg contact, as in tests/test_gpu_dof_force.py:
    nothing touches the robot), one substep with BEZ_FLAG_DOF_FORCE: the call on the PRE-step state (restored with the setters) with udot = (u1 - u0) / h gives DOF_FORCE
    on rows 6:24 and zero on rows 0:6.  The project measured 6.7e-6 N m for the joint rows with the fp64 RNEA."""
    from tests.sim_adapter import SimAdapter
    from tests.scenarios import _free_space_cfg, _pressed_state
    n = 64
    cfg = _free_space_cfg(n, substeps=1)
    cfg.flags |= abi.FLAG_NO_SELF_COLLISION | abi.FLAG_DOF_FORCE
    monkeypatch.setenv("BEZ_SIM_KERNEL", kernel)
    sim = SimAdapter(cfg)
    sim.step(np.zeros((n, 18), np.float32))
    acts = DF.inject_pressed(sim, n, model, 21, _pressed_state)
    rs0, ds0 = sim.root_states.copy(), sim.dof_state.copy()
    sim.pre_physics(acts); sim.simulate()
    rs1, ds1 = sim.root_states.copy(), sim.dof_state.copy()
    sim.sim.refresh_actuator_tensors()
    net = _host(sim.sim.actuator_tensor(abi.ACTUATOR_DOF_FORCE)).reshape(n, 18)
    h = float(cfg.dt) / int(cfg.substeps)
    u0 = np.concatenate([rs0.reshape(n, 2, 13)[:, 0, 7:13], ds0.reshape(n, 18, 2)[:, :, 1]], axis=1).astype(np.float64)
    u1 = np.concatenate([rs1.reshape(n, 2, 13)[:, 0, 7:13], ds1.reshape(n, 18, 2)[:, :, 1]], axis=1).astype(np.float64)
    udot = ((u1 - u0) / h).astype(np.float32)
    sim.set_root_states(rs0.reshape(-1, 13)); sim.set_dof_state(ds0.reshape(-1, 2))
    np.testing.assert_array_equal(sim.dof_state, ds0)
    out = _call(sim.sim, _dev(udot).view(n, NG), abi.ID_ALL).astype(np.float64)
    worst = (float(np.abs(out[:, 0:3]).max()), float(np.abs(out[:, 3:6]).max()), float(np.abs(out[:, 6:] - net).max()))
    print("ID_CLOSURE kernel=%s worst |force| %.3g N, |moment| %.3g N m, |joint rows - DOF_FORCE| %.3g N m (fp64 RNEA on the same identity: 6.7e-6); "
          "largest |DOF_FORCE| %.3g, largest |M udot| row %.3g" % ((kernel,) + worst + (float(np.abs(net).max()),
                                                                    float(np.abs(_call(sim.sim, _dev(udot).view(n, NG), abi.ID_INERTIA)).max()))))
    assert np.abs(net).max() > 0.1 and np.abs(udot).max() > 10   # not vacuous: saturated drives, accelerations of tens of rad/s^2
    assert worst[2] < 2e-2 and worst[0] < 2e-2 and worst[1] < 2e-2, worst


@pytest.mark.parametrize("asset", list(ASSETS))
def test_exact_structure(asset):
    """a dropped or vanishing input leaves exact zeros; the gravity term's force rows are minus the total weight"""
    st = _states()
    n = 65
    cfg = make_cfg(n, seed=5, **ASSETS[asset])
    sim, udot = _prepared(cfg, n, False)
    # velocity term at rest
    root, dof = st["root"][:n].copy(), st["dof"][:n].copy()
    parts = [_call(sim, udot, t) for t in (abi.ID_INERTIA, abi.ID_VELOCITY, abi.ID_GRAVITY)]
    assert not (_bits(_call(sim, None, abi.ID_INERTIA)) << 1).any()          # udot_dev = NULL   (<< 1: up to the sign of zero)
    grav = parts[2]
    Mt = sim.dynamics_tensor("mass_matrix")
    sim.refresh_dynamics_tensors("mass_matrix")
    m00 = _host(Mt)[:, 0, 0]
    g = np.asarray(list(cfg.gravity), np.float32)
    want = -(m00[:, None] * g[None, :])
    assert (np.abs(grav[:, 0:3].astype(np.float64) - want) <= 4.0 * ulp32(want)).all(), np.abs(grav[:, 0:3] - want).max()
    root[:, 7:13] = 0; dof[:, :, 1] = 0
    _write_states(sim, root, dof, st["ball"][:n])
    assert not (_bits(_call(sim, udot, abi.ID_VELOCITY)) << 1).any()          # u = 0
    sim.set_env_params(abi.PARAM_GRAVITY, _dev(np.zeros((n, 3), np.float32)))
    assert not (_bits(_call(sim, udot, abi.ID_GRAVITY)) << 1).any()           # a zero gravity row
    assert np.abs(_call(sim, udot, abi.ID_ALL) - parts[0]).max() < 1e-3        # ... and what is left is the inertia term
    sim.close()


@pytest.mark.parametrize("asset", list(ASSETS))
def test_terms_add_up(asset):
    """All terms together minus the sum of the three single-term calls, per element, within 4 fp32 ulps of sum |terms| of that element.
    The kernel carries the three terms apart and adds them last, so the residual is the rounding of two additions: measured 1.00 ulp on
    MI355X.  (A kernel that adds the terms' accelerations and wrenches link by link misses this by 1400 ulps: the wrenches that cancel
    along a chain to a small joint torque are then rounded at the size of the largest term's.)"""
    n = 65
    sim, udot = _prepared(make_cfg(n, seed=5, **ASSETS[asset]), n, False)
    parts = [_call(sim, udot, t).astype(np.float64) for t in (abi.ID_INERTIA, abi.ID_VELOCITY, abi.ID_GRAVITY)]
    both = _call(sim, udot, abi.ID_ALL).astype(np.float64)
    sim.close()
    total = sum(np.abs(p) for p in parts)
    resid = np.abs(both - sum(parts))
    ratio = resid / ulp32(total)
    e, k = np.unravel_index(np.argmax(ratio), ratio.shape)
    block = np.zeros_like(total)
    for _, sl in ID.BLOCKS:
        block[:, sl] = total[:, sl].max(axis=1, keepdims=True)
    print("ID_ADDITIVE %s worst |all - sum of terms| = %.2f ulps of sum |terms| at env %d row %d (residual %.3g, terms %s); against the ulp of the "
          "block's largest sum |terms| in the env: %.2f ulps" % (asset, ratio[e, k], e, k, resid[e, k], [float(p[e, k]) for p in parts],
                                                                 float((resid / ulp32(block)).max())))
    assert (resid <= 4.0 * ulp32(total)).all(), float(ratio.max())


def test_contract():
    """bad `terms` and a null out: rc -1 with a message that names the function; ten calls allocate nothing; the sim's state is untouched;
    a side stream gives the same bits; the Python layer checks what it is handed"""
    from bez_isaacgym_amd.sim import BezSimError
    n = 65
    sim, udot = _prepared(make_cfg(n, seed=2), n, False)
    out = torch.zeros(n, NG, device="cuda:0")
    torch.cuda.synchronize()
    raw = lambda terms, o: sim.lib.bez_sim_inverse_dynamics(sim.h, C.c_void_p(udot.data_ptr()), terms, o, None)
    for terms, o in ((0, C.c_void_p(out.data_ptr())), (8, C.c_void_p(out.data_ptr())), (1 << 31, C.c_void_p(out.data_ptr())), (9, C.c_void_p(out.data_ptr())),
                     (abi.ID_ALL, None)):
        assert raw(terms, o) == -1, terms
        assert b"bez_sim_inverse_dynamics" in sim.lib.bez_sim_last_error(sim.h)
    assert not out.any()
    snap = lambda: [_host(sim.refresh(w)) for w in (abi.TENSOR_ROOT_STATE, abi.TENSOR_DOF_STATE, abi.TENSOR_DOF_TARGET)]
    state = snap()
    want = _call(sim, udot, abi.ID_ALL)
    before = _free()
    for k in range(10):
        sim.inverse_dynamics(udot if k % 2 else None, TERMS[k % 4], out if k % 3 else None)
    assert _free() == before
    for a, b in zip(state, snap()):
        np.testing.assert_array_equal(_bits(a), _bits(b))
    assert raw(abi.ID_ALL, C.c_void_p(out.data_ptr())) == 0
    np.testing.assert_array_equal(_bits(_host(out)), _bits(want))
    out.zero_()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        sim.inverse_dynamics(udot, abi.ID_ALL, out)
    np.testing.assert_array_equal(_bits(_host(out)), _bits(want))
    assert np.abs(want).max() > 1
    # a view that is contiguous but only 4-byte aligned takes the kernel's scalar path: same bits
    pad = torch.zeros(n * NG + 1, device="cuda:0")
    pad_u, pad_o = torch.zeros(n * NG + 1, device="cuda:0"), pad[1:].view(n, NG)
    pad_u[1:] = udot.reshape(-1)
    sim.inverse_dynamics(pad_u[1:].view(n, NG), abi.ID_ALL, pad_o)
    np.testing.assert_array_equal(_bits(_host(pad_o)), _bits(want))
    for bad in (dict(udot=udot[:, :23]), dict(udot=udot.double()), dict(udot=udot.cpu()), dict(udot=udot.t().contiguous().t()), dict(out=out[:-1]),
                dict(out=out.reshape(-1)), dict(udot=_host(udot)), dict(terms=0), dict(terms=16)):
        with pytest.raises(BezSimError):
            sim.inverse_dynamics(**bad)
    sim.close()


def test_call_captures_into_a_graph():
    """captured once, replayed after the state and udot changed in place, it gives what a direct call gives"""
    n = 65
    st = _states()
    sim = _sim(make_cfg(n, seed=2))
    udot = torch.zeros(n, NG, device="cuda:0")
    out = torch.zeros(n, NG, device="cuda:0")
    sim.inverse_dynamics(udot, abi.ID_ALL, out)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        sim.inverse_dynamics(udot, abi.ID_ALL, out)
    _write_states(sim, st["root"][:n], st["dof"][:n], st["ball"][:n])
    udot.copy_(_dev(st["udot"][:n]).view(n, NG))
    g.replay()
    got = _host(out)
    direct = _call(sim, udot, abi.ID_ALL)
    np.testing.assert_array_equal(_bits(got), _bits(direct))
    assert np.abs(got[:, 0:3]).max() > 10
    sim.close()


def test_vec_task_methods():
    """VecTask.bias_forces() equals the ctypes-level call and has shape (N, 24); gravity_forces and inverse_dynamics likewise"""
    from bez_isaacgym_amd.utils.config import load_config
    from bez_isaacgym_amd.utils.rlgames_utils import get_rlgames_env_creator
    n = 64
    cfg = load_config(["task=bez_kick", "num_envs=%d" % n, "headless=True"])
    env = get_rlgames_env_creator(cfg["task"], "bez_kick", "cuda:0", "cuda:0", 0, True)()
    env.step(torch.rand(n, 18, device=env.device) * 2 - 1)
    out = torch.zeros(n, NG, device=env.device)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    udot = torch.rand(n, NG, device=env.device) * 20 - 10
    for got, terms, u in ((lambda: env.bias_forces(), abi.ID_VELOCITY | abi.ID_GRAVITY, None), (lambda: env.gravity_forces(), abi.ID_GRAVITY, None),
                          (lambda: env.inverse_dynamics(udot), abi.ID_ALL, udot), (lambda: env.inverse_dynamics(udot, abi.ID_INERTIA), abi.ID_INERTIA, udot)):
        assert env.sim.lib.bez_sim_inverse_dynamics(env.sim.h, None if u is None else C.c_void_p(u.data_ptr()), terms, C.c_void_p(out.data_ptr()), stream) == 0
        t = got()
        assert tuple(t.shape) == (n, NG) and t.dtype == torch.float32
        np.testing.assert_array_equal(_bits(_host(t)), _bits(_host(out)))
    b = _host(env.bias_forces())
    assert np.isfinite(b).all() and (b[:, 2] > 20).all()   # the weight, about 25 N, held up
