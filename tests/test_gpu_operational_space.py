"""GPU: bez_sim_operational_space (include/bez_sim.h "Operational space": J_c, J_c M^-1, W = J_E M^-1 J_E^T, Lambda_c = W_cc^-1 of the five
controlled frames) against the fp64 reference of tests/operational_space_numpy.py, against its siblings on the GPU, and its own contract
to the bit.

Sizes: 1, 65 and, around the kernel's 16-env tile, 15, 16, 17; 300 for the known answer alone.  No outlier budget anywhere: every element
of every env is held to its bar.

  known answer   per output and unit class (jac: linear / angular rows; jminv: linear / angular rows x columns 0:3, 3:6, 6:24; w and
                 lambda: lin-lin, lin-ang, ang-ang): 3x the worst absolute error in the class of op_space_ref evaluated in np.float32
                 against fp64 on the same states + 2 fp32 ulps of the class's largest |reference|.
  siblings       at offset 0, two fp32 evaluations of one fp64 quantity: the difference is held to the sum of both sides' bars, each the
                 known-answer bar of the class (the sibling's yardstick is the same dense fp32 evaluation); the push response takes the
                 bars of w through |F|.

Measured on MI355X: known answer, worst error / bar over the six cases 0.99 (cleats, mass-scale rows, jminv angular rows x
columns 0:3), jac 0.45, w 0.65, lambda 0.86; siblings 0.18 at worst, the push response 0.11; J Jbar - I 0.006 of its bar."""
import ctypes as C

import numpy as np
import pytest
import torch

from bez_isaacgym_amd import abi
from tests import dynamics_numpy as D
from tests import limb_ik_numpy as IK
from tests import operational_space_numpy as OS
from tests.gpu_util import ASSETS, _bits, _dev, _free, _host, _prepared, _sim, _states, _write_states
from tests.sim_cfg import make_cfg

pytestmark = pytest.mark.gpu

TILE = 16
SIZES = (1, TILE - 1, TILE, TILE + 1, 65)
NMAX = 300
NG, NCH, NF = abi.NUM_GEN, abi.IK_CHAINS, 6 * abi.IK_CHAINS
OFFSETS = [[0, 0, .03], [0, 0, -.05], [.02, 0, -.01], [0, 0, -.05], [.02, 0, -.01]]
NAMES = ("jac", "jminv", "w", "lambda")
_CACHE = {}


def _refs(asset, randomized, armature):
    """{(fixed, offsets given): (fp64 reference of NMAX envs, {class: bar})} of an asset's link model; computed once per key and left
    unchanged"""
    key = ("ref", "cleats" if asset == "cleats" else "stl", randomized)
    if key not in _CACHE:
        st = _states()
        model, scale = D.model_of(asset), st["scale"] if randomized else None
        M = {f: OS.mass_matrices(model, st["root"], st["dof"], scale, armature, f) for f in (np.float64, np.float32)}
        out = {}
        for fixed in (False, True):
            for off in (False, True):
                r = {f: OS.op_space_ref(model, st["root"], st["dof"], OFFSETS if off else None, scale, armature, fixed, f, M=M[f]) for f in M}
                out[fixed, off] = (r[np.float64], OS.class_bars(r[np.float64], r[np.float32], fixed))
        _CACHE[key] = out
    return _CACHE[key]


def _call(sim, offsets=None, fixed=False, want=None, **kw):
    """{output name: host array or None}"""
    want = (NAMES[:3] if fixed else NAMES) if want is None else want
    return {k: None if t is None else _host(t) for k, t in zip(NAMES, sim.operational_space(offsets, fixed, want=want, **kw))}


def _same_bits(a, b, names=NAMES):
    for k in names:
        if a[k] is not None and b[k] is not None:
            np.testing.assert_array_equal(_bits(a[k]), _bits(b[k]), err_msg=k)


@pytest.mark.parametrize("randomized", [False, True], ids=["default_params", "mass_scale_rows"])
@pytest.mark.parametrize("asset", list(ASSETS))
def test_known_answer(asset, randomized):
    """floating and fixed base, offsets zero and the issue's, against op_space_ref in fp64 on the fp32 states, every element of every env,
    with the default parameters and with a random BEZ_PARAM_MASS_SCALE row (0.5 to 1.5 per link) per env"""
    cfg = lambda n: make_cfg(n, seed=5, **ASSETS[asset])
    refs = _refs(asset, randomized, float(cfg(1).armature))
    report = {}
    for n in SIZES + (NMAX,):
        sim, _ = _prepared(cfg(n), n, randomized)
        for (fixed, off), (ref, bars) in refs.items():
            got = _call(sim, OFFSETS if off else None, fixed)
            for k in NAMES[:3]:
                assert got[k].shape == ref[k][:n].shape and got[k].dtype == np.float32
            for name, v in OS.class_ratios(got, ref, bars, fixed).items():
                report[fixed, off, name] = max(report.get((fixed, off, name), 0.0), v)
        sim.close()
    worst = {}
    for (fixed, off, name), v in report.items():
        worst[name] = max(worst.get(name, 0.0), v)
    print("OS_KNOWN_ANSWER worst error / bar per class:", asset, "randomized" if randomized else "default", {k: round(v, 3) for k, v in worst.items()},
          "bars (floating, offsets):", {k: float("%.3g" % v) for k, v in refs[False, True][1].items()})
    assert max(report.values()) <= 1.0, {k: round(v, 3) for k, v in report.items() if v > 1.0}


@pytest.mark.parametrize("asset", list(ASSETS))
def test_exact_structure(asset):
    """w and lambda are bitwise symmetric; the structural ones and zeros of jac are exact; the fixed base gives its +0.0f pattern; moving
    one chain's offset moves no bit of the blocks that do not involve that chain; an output asked for alone has the bits it has when
    all four are asked for"""
    n = 65
    sim, _ = _prepared(make_cfg(n, seed=5, **ASSETS[asset]), n, True)
    full = _call(sim, OFFSETS)
    assert all(np.isfinite(full[k]).all() for k in NAMES)
    np.testing.assert_array_equal(_bits(full["w"]), _bits(full["w"].transpose(0, 2, 1)))
    np.testing.assert_array_equal(_bits(full["lambda"]), _bits(full["lambda"].transpose(0, 1, 3, 2)))
    J = full["jac"]
    eye = np.broadcast_to(np.eye(3, dtype=np.float32), (n, NCH, 3, 3))
    np.testing.assert_array_equal(_bits(J[:, :, 0:3, 0:3]), _bits(eye))
    np.testing.assert_array_equal(_bits(J[:, :, 3:6, 3:6]), _bits(eye))
    assert not _bits(J[:, :, 3:6, 0:3]).any()
    K = J[:, :, 0:3, 3:6]
    assert not _bits(K[:, :, [0, 1, 2], [0, 1, 2]]).any()
    np.testing.assert_array_equal(_bits(K + np.float32(0)), _bits(-K.transpose(0, 1, 3, 2) + np.float32(0)))   # (a component that is 0 may carry either sign)
    assert np.abs(K).max() > 0.05
    for c, (lo, hi) in enumerate(abi.IK_CHAIN_DOFS):
        other = np.ones(NG, bool); other[0:6] = False; other[6 + lo:6 + hi] = False
        assert not _bits(J[:, c][:, :, other]).any()
        assert np.abs(J[:, c, :, 6 + lo:6 + hi]).max(axis=(0, 1)).min() > 0
    # the fixed base
    fx = _call(sim, OFFSETS, True)
    _same_bits(fx, full, ("jac",))
    assert not _bits(fx["jminv"][..., 0:6]).any()
    blockdiag = np.kron(np.eye(NCH, dtype=bool), np.ones((6, 6), bool))
    assert not _bits(fx["w"][:, ~blockdiag]).any() and np.abs(fx["w"][:, blockdiag]).max() > 1
    np.testing.assert_array_equal(_bits(fx["w"]), _bits(fx["w"].transpose(0, 2, 1)))
    for c, (lo, hi) in enumerate(abi.IK_CHAIN_DOFS):
        other = np.ones(NG, bool); other[6 + lo:6 + hi] = False
        assert not _bits(fx["jminv"][:, c][:, :, other]).any()
    # one chain's offset
    for mode_fixed, base in ((False, full), (True, fx)):
        for c in (1, 4):
            moved = [list(r) for r in OFFSETS]
            moved[c] = [0.05, -0.02, 0.04]
            got = _call(sim, moved, mode_fixed)
            keep = np.arange(NCH) != c
            for k in ("jac", "jminv") + (() if mode_fixed else ("lambda",)):
                np.testing.assert_array_equal(_bits(got[k][:, keep]), _bits(base[k][:, keep]))
                assert (_bits(got[k][:, c]) != _bits(base[k][:, c])).any()
            kk = np.repeat(keep, 6)
            np.testing.assert_array_equal(_bits(got["w"][:, kk][:, :, kk]), _bits(base["w"][:, kk][:, :, kk]))
            assert (_bits(got["w"][:, ~kk]) != _bits(base["w"][:, ~kk])).any()
    # one output alone, into the caller's tensor
    for k in NAMES:
        t = torch.full(full[k].shape, 7.0, device="cuda:0")
        alone = _call(sim, OFFSETS, False, (), **{"lam" if k == "lambda" else k: t})
        assert [x for x in NAMES if alone[x] is not None] == [k]
        _same_bits(alone, full, (k,))
    _same_bits(_call(sim, OFFSETS, True, ("w",)), fx, ("w",))
    sim.close()


@pytest.mark.parametrize("asset", list(ASSETS))
def test_against_the_siblings(asset):
    """offset 0, a mass-scale row per env: jac against the refreshed Jacobian tensor's rows of the end bodies; row i of jminv[c] against
    forward_dynamics(jac[:, c, i, :], bias = 0); w[:, :, c-block] @ F against body_accelerations(forward_dynamics(generalized_forces(F at
    the origin of end body c), 0), ACC_UDOT) at every end body"""
    n = 65
    cfg = make_cfg(n, seed=5, **ASSETS[asset])
    ref, bars = _refs(asset, True, float(cfg.armature))[False, False]
    sim, _ = _prepared(cfg, n, True)
    model = D.model_of(asset)
    ends = [IK.end_body(model, c) for c in range(NCH)]
    nb = sim.num_bodies - (1 if sim.has_ball else 0)
    jac_t, jminv_t, w_t, _ = sim.operational_space()
    jac, jminv, w = _host(jac_t), _host(jminv_t), _host(w_t).astype(np.float64)
    cls = OS.classes()
    Jt = sim.dynamics_tensor("jacobian")
    sim.refresh_dynamics_tensors("jacobian")
    Jrows = _host(Jt).reshape(n, nb, 6, NG)[:, ends]
    report = {}
    for name in ("jac_lin", "jac_ang"):
        m = cls[name][1]
        report[name] = float(np.abs(jac.astype(np.float64)[:, m] - Jrows.astype(np.float64)[:, m]).max() / (2.0 * bars[name]))
    solved = np.zeros_like(jminv)
    for c in range(NCH):
        for i in range(6):
            solved[:, c, i] = _host(sim.forward_dynamics(jac_t[:, c, i, :].contiguous(), 0))
    for name in [k for k in cls if k.startswith("jminv_")]:
        m = cls[name][1]
        report[name] = float(np.abs(jminv.astype(np.float64)[:, m] - solved.astype(np.float64)[:, m]).max() / (2.0 * bars[name]))
    # the push response
    wbar = np.zeros((NF, NF))
    for name in ("w_lin_lin", "w_lin_ang", "w_ang_ang"):
        wbar[cls[name][1]] = bars[name]
    rng = np.random.default_rng(77)
    push = 0.0
    for c in range(NCH):
        F = (rng.uniform(-1, 1, (n, 6)) * np.array([5.0, 5.0, 5.0, 0.5, 0.5, 0.5])).astype(np.float32)
        forces, torques = np.zeros((n, sim.num_bodies, 3), np.float32), np.zeros((n, sim.num_bodies, 3), np.float32)
        forces[:, ends[c]], torques[:, ends[c]] = F[:, 0:3], F[:, 3:6]
        f = sim.generalized_forces(_dev(forces).view(n, -1, 3), _dev(torques).view(n, -1, 3), at="origin")
        acc = _host(sim.body_accelerations(sim.forward_dynamics(f, 0), abi.ACC_UDOT))[:, ends].reshape(n, NF).astype(np.float64)
        mine = np.einsum("nij,nj->ni", w[:, :, 6 * c:6 * c + 6], F.astype(np.float64))
        bar = 2.0 * np.einsum("ij,nj->ni", wbar[:, 6 * c:6 * c + 6], np.abs(F).astype(np.float64))
        want = np.einsum("nij,nj->ni", ref["w"][:n, :, 6 * c:6 * c + 6], F.astype(np.float64))
        assert np.abs(want).max() > 1
        push = max(push, float((np.abs(mine - acc) / bar).max()))
    report["push"] = push
    sim.close()
    print("OS_SIBLINGS worst difference / (sum of both bars):", asset, {k: round(v, 3) for k, v in report.items()})
    assert max(report.values()) <= 1.0, report


def test_bits_do_not_depend_on_the_number_of_envs():
    """env e of the N = 65 run has the bits of env e of every smaller run, floating and fixed"""
    cfg = lambda n: make_cfg(n, seed=5)
    modes = (False, True)
    sim, _ = _prepared(cfg(max(SIZES)), max(SIZES), True)
    big = [_call(sim, OFFSETS, f) for f in modes]
    sim.close()
    for n in SIZES[:-1]:
        sim, _ = _prepared(cfg(n), n, True)
        for f, want in zip(modes, big):
            got = _call(sim, OFFSETS, f)
            _same_bits(got, {k: None if v is None else v[:n] for k, v in want.items()})
        sim.close()


def test_a_nan_stays_in_its_env():
    """N = 17: a NaN in one env's q -- every other env has the bits of the clean run and every output of the poisoned env is not finite"""
    n, bad = TILE + 1, 5
    st = _states()
    sim, _ = _prepared(make_cfg(n, seed=5), n, True)
    clean = [_call(sim, OFFSETS, f) for f in (False, True)]
    assert all(np.isfinite(v).all() for c in clean for v in c.values() if v is not None)
    dof = st["dof"][:n].copy()
    dof[bad, 7, 0] = np.nan
    _write_states(sim, st["root"][:n], dof, st["ball"][:n])
    keep = np.arange(n) != bad
    for f, want in zip((False, True), clean):
        got = _call(sim, OFFSETS, f)
        for k in NAMES:
            if got[k] is not None:
                np.testing.assert_array_equal(_bits(got[k][keep]), _bits(want[k][keep]))
                assert not np.isfinite(got[k][bad]).all(), k
    sim.close()


def test_contract():
    """every rc -1 case names the function and leaves the sentinel-filled outputs untouched; ten calls allocate nothing; the sim's state is
    untouched; a side stream and 4-byte-aligned views give the same bits; the Python layer checks what it is handed"""
    from bez_isaacgym_amd.sim import BezSimError
    n = 65
    sim, _ = _prepared(make_cfg(n, seed=2), n, False)
    shapes = {"jac": (n, NCH, 6, NG), "jminv": (n, NCH, 6, NG), "w": (n, NF, NF), "lambda": (n, NCH, 6, 6)}
    outs = {k: torch.full(s, 7.0, device="cuda:0") for k, s in shapes.items()}
    torch.cuda.synchronize()
    ptr = {k: C.c_void_p(t.data_ptr()) for k, t in outs.items()}
    good, fixed = abi.op_space_params(OFFSETS), abi.op_space_params(OFFSETS, True)
    badmode = abi.op_space_params(OFFSETS); badmode.mode = 2
    badmode2 = abi.op_space_params(OFFSETS); badmode2.mode = 1 | (1 << 31)
    nan = abi.op_space_params(OFFSETS); nan.offset[3][1] = float("nan")
    inf = abi.op_space_params(OFFSETS); inf.offset[0][0] = float("-inf")
    raw = lambda h, p, a, b, c, d: sim.lib.bez_sim_operational_space(h, None if p is None else C.byref(p), a, b, c, d, None)
    allp = [ptr[k] for k in NAMES]
    for args in ((sim.h, None, *allp), (sim.h, good, None, None, None, None), (sim.h, badmode, *allp), (sim.h, badmode2, *allp), (sim.h, nan, *allp),
                 (sim.h, inf, *allp), (sim.h, fixed, *allp), (sim.h, fixed, None, None, None, ptr["lambda"])):
        assert raw(*args) == -1
        assert b"bez_sim_operational_space" in sim.lib.bez_sim_last_error(sim.h)
    assert raw(None, good, *allp) == -1 and b"bez_sim_operational_space" in sim.lib.bez_sim_last_error(None)
    torch.cuda.synchronize()
    assert all(bool((t == 7.0).all()) for t in outs.values())
    snap = lambda: [_host(sim.refresh(w)) for w in (abi.TENSOR_ROOT_STATE, abi.TENSOR_DOF_STATE, abi.TENSOR_DOF_TARGET)]
    state = snap()
    want = _call(sim, OFFSETS)
    want_fx = _call(sim, OFFSETS, True)
    before = _free()
    for k in range(10):
        sim.operational_space(OFFSETS if k % 2 else None, bool(k % 3 == 0), want=NAMES[k % 3:3] if k % 3 == 0 else NAMES[k % 4:])
    assert _free() == before
    for a, b in zip(state, snap()):
        np.testing.assert_array_equal(_bits(a), _bits(b))
    assert raw(sim.h, good, *allp) == 0
    _same_bits({k: _host(t) for k, t in outs.items()}, want)
    for t in outs.values():
        t.fill_(7.0)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        sim.operational_space(OFFSETS, False, outs["jac"], outs["jminv"], outs["w"], outs["lambda"])
    _same_bits({k: _host(t) for k, t in outs.items()}, want)
    # views that are contiguous but only 4-byte aligned take the kernel's scalar path: same bits
    pads = {k: torch.zeros(int(np.prod(s)) + 1, device="cuda:0") for k, s in shapes.items()}
    views = {k: pads[k][1:].view(shapes[k]) for k in shapes}
    assert all(v.data_ptr() % 16 == 4 for v in views.values())
    sim.operational_space(OFFSETS, False, views["jac"], views["jminv"], views["w"], views["lambda"])
    _same_bits({k: _host(v) for k, v in views.items()}, want)
    sim.operational_space(OFFSETS, True, views["jac"], views["jminv"], views["w"], want=())
    _same_bits({k: _host(views[k]) for k in NAMES[:3]}, want_fx, NAMES[:3])
    w = outs["w"]
    for bad in (dict(w=w[:, :29]), dict(w=w.double()), dict(w=w.cpu()), dict(w=w.transpose(1, 2)), dict(jac=outs["jac"][:-1]), dict(jminv=outs["jac"].reshape(n, -1)),
                dict(lam=outs["w"]), dict(jac=_host(outs["jac"])), dict(want=("jac", "lam")), dict(want=()), dict(offsets=OFFSETS[:4]),
                dict(offsets=[[float("nan")] * 3] * 5), dict(fixed_base=True), dict(fixed_base=True, want=("lambda",)), dict(fixed_base=True, want=("w",), lam=outs["lambda"])):
        with pytest.raises(BezSimError):
            sim.operational_space(**bad)
    sim.close()


def test_call_captures_into_a_graph():
    """captured once, replayed after the state changed in place, it gives what a direct call gives"""
    n = 65
    st = _states()
    sim = _sim(make_cfg(n, seed=2))
    shapes = {"jac": (n, NCH, 6, NG), "jminv": (n, NCH, 6, NG), "w": (n, NF, NF), "lambda": (n, NCH, 6, 6)}
    outs = {k: torch.zeros(s, device="cuda:0") for k, s in shapes.items()}
    call = lambda: sim.operational_space(OFFSETS, False, outs["jac"], outs["jminv"], outs["w"], outs["lambda"])
    call()
    torch.cuda.synchronize()
    before = {k: _host(t) for k, t in outs.items()}
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call()
    _write_states(sim, st["root"][:n], st["dof"][:n], st["ball"][:n])
    g.replay()
    got = {k: _host(t) for k, t in outs.items()}
    _same_bits(got, _call(sim, OFFSETS))
    assert all((_bits(got[k]) != _bits(before[k])).any() for k in NAMES)
    sim.close()


def test_vec_task_methods():
    """the VecTask helpers equal the ctypes-level call on a stepped bez_kick env of 64; J_c Jbar_c = I within the bars of jminv and lambda
    taken through the two products"""
    from bez_isaacgym_amd.utils.config import load_config
    from bez_isaacgym_amd.utils.rlgames_utils import get_rlgames_env_creator
    n = 64
    cfg = load_config(["task=bez_kick", "num_envs=%d" % n, "headless=True"])
    env = get_rlgames_env_creator(cfg["task"], "bez_kick", "cuda:0", "cuda:0", 0, True)()
    env.step(torch.rand(n, 18, device=env.device) * 2 - 1)
    assert not int(env.sim.cfg.flags) & abi.FLAG_FIX_BASE
    shapes = {"jac": (n, NCH, 6, NG), "jminv": (n, NCH, 6, NG), "w": (n, NF, NF), "lambda": (n, NCH, 6, 6)}
    outs = {k: torch.zeros(s, device=env.device) for k, s in shapes.items()}
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    raw = lambda mode, names: env.sim.lib.bez_sim_operational_space(env.sim.h, C.byref(abi.op_space_params(OFFSETS, mode)),
                                                                    *[C.c_void_p(outs[k].data_ptr()) if k in names else None for k in NAMES], stream)
    assert raw(False, NAMES) == 0
    want = {k: _host(t) for k, t in outs.items()}
    got = dict(zip(NAMES, env.operational_space(OFFSETS)))
    _same_bits({k: _host(t) for k, t in got.items()}, want)
    for k, t in (("jac", env.end_effector_jacobian(OFFSETS)), ("w", env.delassus_matrix(OFFSETS)), ("lambda", env.operational_space_inertia(OFFSETS))):
        assert tuple(t.shape) == shapes[k] and t.dtype == torch.float32
        np.testing.assert_array_equal(_bits(_host(t)), _bits(want[k]))
    assert raw(True, NAMES[:3]) == 0
    fx = dict(zip(NAMES, env.operational_space(OFFSETS, fixed_base=True, want=NAMES[:3])))
    assert fx["lambda"] is None
    _same_bits({k: _host(fx[k]) for k in NAMES[:3]}, {k: _host(outs[k]) for k in NAMES[:3]}, NAMES[:3])
    jbar = env.dynamically_consistent_inverse(OFFSETS)
    assert tuple(jbar.shape) == (n, NCH, NG, 6)
    lam, jminv, jac = want["lambda"].astype(np.float64), want["jminv"].astype(np.float64), want["jac"].astype(np.float64)
    np.testing.assert_array_equal(_bits(_host(jbar)), _bits(_host(torch.matmul(_dev(want["lambda"]).view(n, NCH, 6, 6), _dev(want["jminv"]).view(n, NCH, 6, NG)).transpose(-1, -2))))
    # J_c Jbar_c = (Lambda_c W_cc)^T: the bars of jminv and lambda through the products, on the default model's states of the known answer
    _, bars = _refs("default", False, float(env.sim.cfg.armature))[False, True]
    cls = OS.classes()
    bj, bl, bjac = np.zeros((NCH, 6, NG)), np.zeros((NCH, 6, 6)), np.zeros((NCH, 6, NG))
    for name, (o, m) in cls.items():
        if o in ("jminv", "lambda", "jac"):
            {"jminv": bj, "lambda": bl, "jac": bjac}[o][m] = bars[name]
    prod = np.einsum("ncik,nckj->ncij", jac, _host(jbar).astype(np.float64))
    A = np.einsum("ncik,nclk->ncil", jac, jminv)                               # J M^-1 J^T = W_cc
    bar = np.einsum("ncil,clj->ncij", np.abs(A), bl) + np.einsum("ncik,clk,nclj->ncij", np.abs(jac), bj, np.abs(lam)) \
        + np.einsum("cik,nclk,nclj->ncij", bjac, np.abs(jminv), np.abs(lam)) \
        + 32 * 2.0 ** -24 * np.einsum("ncik,nclk,nclj->ncij", np.abs(jac), np.abs(jminv), np.abs(lam))
    ratio = np.abs(prod - np.eye(6)) / bar
    print("OS_VEC_TASK worst |J Jbar - I| %.3g, / bar %.3g" % (np.abs(prod - np.eye(6)).max(), ratio.max()))
    assert (ratio <= 1.0).all(), float(ratio.max())
