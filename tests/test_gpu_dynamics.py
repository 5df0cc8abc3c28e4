"""GPU: the dynamics tensors (include/bez_sim.h "Dynamics tensors": the robot's Jacobian (N*NB, 6, 24) and mass matrix (N, 24, 24))
against the fp64 references of tests/dynamics_numpy.py, on the state set of tests/state_sets.py.

Sizes: the rigid-body refresh's 1, 63, 64, 65, 300 and, around the kernel's 16-env tile, 15, 16, 17.  Assets default, cleats, box; the
kick (ball actor) and walk (no ball) layouts.  No outlier budget anywhere: every element of every env is held to its bar.

  J   per field (rows 0:3 linear, 3:6 angular): 3x the fp32 oracle's worst error on the same unit-velocity rows + 2 fp32 ulps of the
      value, as tests/gpu_util._bars builds the rigid-body rows'.
  M   3x the worst error of the sum J^T M J route evaluated in np.float32 against fp64 on the same states + 2 fp32 ulps of
      sqrt(M_ii M_jj); the worst error is the largest absolute one over every element and state, as _bars takes its own.  The error
      relative to each element's own sqrt(M_ii M_jj) is printed beside it as a measurement, not asserted: the kernel's recursion sums
      inertias about the root origin, so a distal joint's entry carries the rounding of m r^2 with r its distance from the ROOT
      (DESIGN.md 4.3e), which the yardstick route -- sums about each link's own centre of mass -- does not have.
  J u against the refreshed RIGID_BODY_STATE[..., 7:13] (both fp32 on the GPU): the fp64-evaluated rounding bound of a 24-term fp32
      dot product, 24 * 2^-23 * sum |J_k| |u_k|, plus the rigid-body test's field bar.

Measured on MI355X, worst error / bar at n = 300 (bez_kick): see DESIGN.md 4.3e."""
import ctypes as C

import numpy as np
import pytest
import torch

from bez_isaacgym_amd import abi
from tests import dynamics_numpy as D
from tests.gpu_util import ASSETS, _J_refs, _bars, _bits, _dev, _free, _host, _ids, _sim, _write_states
from tests.sim_cfg import make_cfg
from tests.state_sets import FIELDS, ball_states, field_errors, generate_states, oracle_rows, ulp32

pytestmark = pytest.mark.gpu

TILE = 16
SIZES = (1, TILE - 1, TILE, TILE + 1, 63, 64, 65, 300)
NMAX = max(SIZES)
NG = abi.NUM_GEN
_CACHE = {}


def _states():
    if "states" not in _CACHE:
        root, dof, _ = generate_states(NMAX)
        scale = np.random.default_rng(17).uniform(0.5, 1.5, (NMAX, 19)).astype(np.float32)
        _CACHE["states"] = dict(root=root, dof=dof, ball=ball_states(NMAX), scale=scale)
    return _CACHE["states"]


def _M_refs(asset, root, dof, scale, armature, key):
    """(fp64 M_ref, the bars, sqrt(M_ii M_jj)) of an asset's link model, `scale` (n, 19) or None"""
    if key not in _CACHE:
        model = D.model_of(asset)
        n = root.shape[0]
        M64, M32 = np.zeros((n, NG, NG)), np.zeros((n, NG, NG))
        for e in range(n):
            s = None if scale is None else scale[e]
            M64[e] = D.M_ref_jtmj(model, root[e, 3:7], dof[e, :, 0], s, armature)
            M32[e] = D.M_ref_jtmj(model, root[e, 3:7], dof[e, :, 0], s, armature, dtype=np.float32)
        size = D.scale_of(M64)
        err = np.abs(M32 - M64)
        bar_abs = 3.0 * float(err.max()) + 2.0 * ulp32(size)
        _CACHE[key] = (M64, bar_abs, size)
    return _CACHE[key]


def _check_J_structure(J, asset):
    """bit-exact: non-ancestor columns 0.0, the base blocks I / I / 0, the imu row equal to the torso's"""
    n, nb = J.shape[:2]
    body_link = D.model_of(asset)["body_link"]
    assert len(body_link) == nb
    links = D.MODEL["links"]
    for b, l in enumerate(body_link):
        anc = np.zeros(18, bool)
        while l > 0:
            anc[l - 1] = True
            l = links[l]["parent"]
        assert (_bits(J[:, b, :, 6:][:, :, ~anc]) == 0).all(), ("non-ancestor columns of body", b)
    eye = np.broadcast_to(np.eye(3, dtype=np.float32), (n, nb, 3, 3))
    np.testing.assert_array_equal(_bits(J[:, :, 0:3, 0:3]), _bits(eye))
    np.testing.assert_array_equal(_bits(J[:, :, 3:6, 3:6]), _bits(eye))
    np.testing.assert_array_equal(_bits(J[:, :, 3:6, 0:3]), _bits(0 * eye))
    np.testing.assert_array_equal(_bits(J[:, 1]), _bits(J[:, 0]))
    np.testing.assert_array_equal(np.abs(J[:, 0, 0:3, 3:6]), 0 * eye[:, 0])   # the torso origin is the root's


def _check(got, ref, bar, what):
    err = np.abs(got.astype(np.float64) - ref)
    bad = err > bar
    assert not bad.any(), (what, float(err.max()), [tuple(x) for x in np.argwhere(bad)[:5]])
    return float((err / bar).max())


@pytest.mark.parametrize("task", ["bez_kick", "bez_walk"])
@pytest.mark.parametrize("asset", list(ASSETS))
def test_jacobian_against_fp64_reference(asset, task):
    """every element of J of every env against J_ref; the bit-exact structure; J u against the refreshed rigid-body rows"""
    st = _states()
    root, dof, ball = st["root"], st["dof"], st["ball"]
    J64, barsJ = _J_refs(asset, root, dof, ("J", asset))
    cfg = lambda n: make_cfg(n, task=task, seed=5, **ASSETS[asset])
    nb = J64.shape[1]
    o64 = oracle_rows(cfg(NMAX), "f64", root, dof, ball)[:, :nb].astype(np.float64)
    o32 = oracle_rows(cfg(NMAX), "f32", root, dof, ball)[:, :nb]
    field = _bars(field_errors(o32, o64), o64)
    u = np.concatenate([root[:, 7:13], dof[:, :, 1]], axis=1).astype(np.float64)
    report = {}
    for n in SIZES:
        sim = _sim(cfg(n))
        _write_states(sim, root[:n], dof[:n], ball[:n])
        Jt = sim.dynamics_tensor("jacobian")
        assert tuple(Jt.shape) == (n * nb, 6, NG) and Jt.dtype == torch.float32 and Jt.is_contiguous()
        sim.refresh_dynamics_tensors("jacobian")
        J = _host(Jt).reshape(n, nb, 6, NG)
        report[n] = _check(J, J64[:n], barsJ[:n], (asset, task, n, "J"))
        _check_J_structure(J, asset)
        rb = _host(sim.refresh(abi.TENSOR_RIGID_BODY_STATE)).reshape(n, -1, 13)[:, :nb]
        Ju = np.einsum("ebrk,ek->ebr", J.astype(np.float64), u[:n])
        dot_bound = NG * 2.0 ** -23 * np.einsum("ebrk,ek->ebr", np.abs(J).astype(np.float64), np.abs(u[:n]))
        for name, sl, rows in (("lin", slice(7, 10), slice(0, 3)), ("ang", slice(10, 13), slice(3, 6))):
            report[n, name] = _check(Ju[..., rows], rb[..., sl].astype(np.float64), dot_bound[..., rows] + field[name][:n], (asset, task, n, "J u", name))
        sim.close()
    print("J: worst error / bar:", asset, task, report)


@pytest.mark.parametrize("scaled", [False, True], ids=["default_params", "mass_scale"])
@pytest.mark.parametrize("task", ["bez_kick", "bez_walk"])
@pytest.mark.parametrize("asset", list(ASSETS))
def test_mass_matrix_against_fp64_reference(asset, task, scaled):
    """every element of M of every env against M_ref, with the default parameters and with a random BEZ_PARAM_MASS_SCALE row per env;
    M == M^T bitwise; the translational block is the total mass times I, exactly"""
    st = _states()
    root, dof, ball = st["root"], st["dof"], st["ball"]
    scale = st["scale"] if scaled else None
    cfg = lambda n: make_cfg(n, task=task, seed=5, **ASSETS[asset])
    M64, bar_abs, size = _M_refs(asset, root, dof, scale, float(cfg(1).armature), ("M", "cleats" if asset == "cleats" else "stl", scaled))
    report = {}
    for n in SIZES:
        sim = _sim(cfg(n))
        _write_states(sim, root[:n], dof[:n], ball[:n])
        if scaled:
            sim.set_env_params(abi.PARAM_MASS_SCALE, _dev(scale[:n]))
        Mt = sim.dynamics_tensor("mass_matrix")
        assert tuple(Mt.shape) == (n, NG, NG) and Mt.dtype == torch.float32
        sim.refresh_dynamics_tensors("mass_matrix")
        M = _host(Mt)
        report[n] = (_check(M, M64[:n], bar_abs[:n], (asset, task, n, "M")), float((np.abs(M - M64[:n]) / size[:n]).max()))
        np.testing.assert_array_equal(_bits(M), _bits(np.swapaxes(M, 1, 2)))
        t = M[:, 0:3, 0:3]
        assert (_bits(t[:, ~np.eye(3, dtype=bool)]) == 0).all()
        assert (t[:, 0, 0] == t[:, 1, 1]).all() and (t[:, 0, 0] == t[:, 2, 2]).all()
        sim.close()
    print("M: (worst error / bar, worst error / sqrt(M_ii M_jj)):", asset, task, "mass_scale" if scaled else "default", report)


def test_after_motion():
    """five steps with seeded random actions at N = 65, then ROOT_STATE, DOF_STATE, J and M refreshed together: J and M against
    references built from the state that was read back, under the same bars"""
    n = 65
    cfg = make_cfg(n, seed=11)
    sim = _sim(cfg)
    rng = np.random.default_rng(3)
    Jt, Mt = sim.dynamics_tensor("jacobian"), sim.dynamics_tensor("mass_matrix")
    for _ in range(5):
        sim.step(_dev(rng.uniform(-1, 1, (n, 18)).astype(np.float32)))
    root = _host(sim.refresh(abi.TENSOR_ROOT_STATE)).reshape(n, 2, 13)[:, 0]
    dof = _host(sim.refresh(abi.TENSOR_DOF_STATE)).reshape(n, 18, 2)
    sim.refresh_dynamics_tensors()
    J, M = _host(Jt).reshape(n, 21, 6, NG), _host(Mt)
    sim.close()
    assert np.isfinite(root).all() and np.abs(dof[:, :, 1]).max() > 0.1
    J64, barsJ = _J_refs("default", root, dof, ("J", "after motion"))
    M64, bar_abs, _ = _M_refs("default", root, dof, None, float(cfg.armature), ("M", "after motion"))
    worst = (_check(J, J64, barsJ, "J after motion"), _check(M, M64, bar_abs, "M after motion"))
    _check_J_structure(J, "default")
    np.testing.assert_array_equal(_bits(M), _bits(np.swapaxes(M, 1, 2)))
    print("after motion: worst error / bar (J, M):", worst)


# ---------------------------------------------------------------- the contract of the two entry points

def test_refresh_contract():
    """refresh before the acquisition, a zero mask and an unknown bit: rc -1 with a message; after the acquisitions ten refreshes leave
    the free device memory unchanged; a refresh on a side stream with one final synchronise gives the same bits"""
    from bez_isaacgym_amd.sim import BezSimError
    n = 65
    st = _states()
    sim = _sim(make_cfg(n, seed=2))
    _write_states(sim, st["root"][:n], st["dof"][:n], st["ball"][:n])
    torch.cuda.synchronize()
    refresh = lambda mask: sim.lib.bez_sim_refresh_dynamics_tensors(sim.h, mask, None)
    for mask in (1, 2, 3, 0, 4, 7, 1 << 31):
        assert refresh(mask) == -1, mask
        assert b"bez_sim_refresh_dynamics_tensors" in sim.lib.bez_sim_last_error(sim.h)
    for call in (lambda: sim.refresh_dynamics_tensors(), lambda: sim.refresh_dynamics_tensors("jacobian"),
                 lambda: sim.refresh_dynamics_tensors(["jacobian", "mass_matrix"])):
        with pytest.raises(BezSimError):
            call()
    Jt = sim.dynamics_tensor("jacobian")
    assert refresh(1) == 0 and refresh(2) == -1 and refresh(3) == -1   # the mass matrix is still not acquired
    Mt = sim.dynamics_tensor(abi.DYNAMICS_MASS_MATRIX)
    assert sim.dynamics_tensor("jacobian").data_ptr() == Jt.data_ptr() and Mt.data_ptr() != Jt.data_ptr()
    for mask in (0, 4, 5, 1 << 31):
        assert refresh(mask) == -1, mask
    p, shape, nd, dt = C.c_void_p(), (C.c_int64 * 3)(), C.c_int(), C.c_int()
    for which in (-1, 2):
        assert sim.lib.bez_sim_get_dynamics_tensor(sim.h, which, C.byref(p), shape, C.byref(nd), C.byref(dt)) == -1
    sim.refresh_dynamics_tensors()
    before = _free()
    for k in range(10):
        sim.refresh_dynamics_tensors([("jacobian",), ("mass_matrix",), ("jacobian", "mass_matrix")][k % 3])
    assert _free() == before
    want = (_host(Jt), _host(Mt))
    Jt.zero_(); Mt.zero_()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        sim.refresh_dynamics_tensors()
    torch.cuda.synchronize()
    np.testing.assert_array_equal(_bits(Jt.cpu().numpy()), _bits(want[0]))
    np.testing.assert_array_equal(_bits(Mt.cpu().numpy()), _bits(want[1]))
    assert np.abs(want[0]).max() > 0 and np.abs(want[1]).max() > 0
    sim.close()


def test_refresh_captures_into_a_graph():
    """the refresh reads nothing on the host: captured once, replayed after the state changed, it gives what a direct call gives"""
    n = 65
    st = _states()
    sim = _sim(make_cfg(n, seed=2))
    Jt, Mt = sim.dynamics_tensor("jacobian"), sim.dynamics_tensor("mass_matrix")
    sim.refresh_dynamics_tensors()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        sim.refresh_dynamics_tensors()
    _write_states(sim, st["root"][:n], st["dof"][:n], st["ball"][:n])
    g.replay()
    got = (_host(Jt), _host(Mt))
    Jt.zero_(); Mt.zero_()
    sim.refresh_dynamics_tensors()
    np.testing.assert_array_equal(_bits(got[0]), _bits(_host(Jt)))
    np.testing.assert_array_equal(_bits(got[1]), _bits(_host(Mt)))
    assert np.abs(got[0][:, 0:3, 3:6]).max() > 0.01
    sim.close()


def test_allocation_is_lazy_and_destroy_returns_it():
    """a sim allocates nothing for these tensors until they are acquired (the acquisition is what moves the free device memory, by the
    tensors' size); create -> acquire both -> destroy leaves the free memory where it was, within what a plain create / destroy moves it"""
    n = 2048
    bytes_J, bytes_M = n * 21 * 6 * NG * 4, n * NG * NG * 4

    def cycle(acquire):
        sim = _sim(make_cfg(n, seed=1))
        created = _free()
        if acquire:
            sim.dynamics_tensor("jacobian"); sim.dynamics_tensor("mass_matrix")
            sim.refresh_dynamics_tensors()
        acquired = _free()
        sim.close()
        return created - acquired

    cycle(True)                      # (code objects and torch's own pool)
    start = _free()
    assert cycle(False) == 0
    granularity = abs(_free() - start)
    taken = cycle(True)
    end = _free()
    print("free device memory: %d before, %d after, granularity %d; the acquisitions took %d for %d bytes" % (start, end, granularity, taken, bytes_J + bytes_M))
    assert taken >= bytes_J + bytes_M - (2 << 20) and taken <= bytes_J + bytes_M + (4 << 20), (taken, bytes_J + bytes_M)
    assert abs(end - start) <= granularity, (start, end, granularity)


def test_vec_task_views_have_the_documented_shapes_and_alias_the_sim():
    from bez_isaacgym_amd.utils.config import load_config
    from bez_isaacgym_amd.utils.rlgames_utils import get_rlgames_env_creator
    n = 64
    cfg = load_config(["task=bez_kick", "num_envs=%d" % n, "headless=True"])
    env = get_rlgames_env_creator(cfg["task"], "bez_kick", "cuda:0", "cuda:0", 0, True)()
    for name in ("jacobian", "mass_matrix"):
        with pytest.raises(AttributeError, match="acquire_%s_tensor" % name):
            getattr(env, name)
        with pytest.raises(AttributeError):
            getattr(env, "refresh_%s" % name + ("_tensors"))()
    J, M = env.acquire_jacobian_tensor(), env.acquire_mass_matrix_tensor()
    assert tuple(J.shape) == (n, 21, 6, 24) and tuple(M.shape) == (n, 24, 24)
    assert env.jacobian.data_ptr() == J.data_ptr() == env.sim.dynamics_tensor("jacobian").data_ptr()
    assert env.mass_matrix.data_ptr() == M.data_ptr() == env.sim.dynamics_tensor("mass_matrix").data_ptr()
    env.step(torch.rand(n, 18, device=env.device) * 2 - 1)
    assert env.refresh_jacobian_tensors() is True and env.refresh_mass_matrix_tensors() is True
    torch.cuda.synchronize()
    assert (J[:, :, 0, 0] == 1).all() and (M[:, 0, 0] > 2).all() and torch.isfinite(J).all() and torch.isfinite(M).all()
    rb = env.sim.refresh(abi.TENSOR_RIGID_BODY_STATE).view(n, 22, 13)[:, :21, 7:13]
    rs = env.sim.refresh(abi.TENSOR_ROOT_STATE).view(n, 2, 13)[:, 0, 7:13]
    qd = env.sim.refresh(abi.TENSOR_DOF_STATE).view(n, 18, 2)[:, :, 1]
    u = torch.cat([rs, qd], dim=1)
    assert (torch.einsum("ebrk,ek->ebr", J, u) - rb).abs().max().item() < 1e-3
