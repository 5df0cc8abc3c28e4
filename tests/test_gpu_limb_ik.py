"""GPU: bez_sim_limb_ik (include/bez_sim.h "Limb inverse kinematics": damped least squares per chain) against the fp64 reference of
tests/limb_ik_numpy.py, against the Jacobian tensor, and its own contract to the bit.

Sizes: 1, 15, 16, 17, 31, 32, 33 (the kernel's 32-env tile, and the 16-env tile of its neighbours), 65 (past a wave), 300 (many tiles,
ragged last tile).  Assets default / cleats / box and box + cleats (the asset whose right ankle's joint origin moves) in the kick and walk
layouts.  No outlier budget anywhere: every element of every env is held to its bar.

  known answer   per block (each chain's q, the position rows, the rotation rows): 3x the worst absolute error of limb_ik_ref evaluated
                 in np.float32 against fp64 on the same inputs + 2 fp32 ulps of the block's largest |reference|.
  convergence    the weighted residual after 30 iterations at the lambda of tests/limb_ik_inputs.CONV against the reference's + the
                 known-answer bars of the error rows taken through the residual's norm.
  duality        dq of one unlimited step against (J^T W J + lambda^2 I)^-1 J^T W e with the refreshed Jacobian tensor's columns in
                 the root's axes, solved in fp64: the Jacobian test's per-entry bar and the bar of the error rows (the iters = 0 call's,
                 whose err_out enters) propagated through the solve to first order, + the known-answer bar of q.  The propagation takes
                 every rounding with the worst sign through |N^-1|, so it is a worst-case bound; that it still tells a wrong solve
                 apart is shown by the same solve with lambda 10 % off, which must miss it.

Measured on MI355X: see DESIGN.md 4.3k and profiles/limb_ik_errors.txt."""
import numpy as np
import pytest
import torch

from bez_isaacgym_amd import abi
from tests import limb_ik_numpy as IK
from tests.gpu_util import ASSETS, _bits, _dev, _host, _sim, _write_states
from tests.limb_ik_inputs import CONV, convergence_inputs
from tests.sim_cfg import make_cfg
from tests.state_sets import ball_states, generate_states, ulp32

pytestmark = pytest.mark.gpu

TILE = 32
SIZES = (1, 15, 16, 17, TILE - 1, TILE, TILE + 1, 65, 300)
NMAX = max(SIZES)
ASSETS4 = dict(ASSETS, box_cleats=dict(cleats=True, box=True))
SPACES = (("env", IK.SPACE_ENV), ("root", IK.SPACE_ROOT))
WEIGHTS = [[1.0, 0.25], [2.0, 0.1], [1.0, 0.5], [0.5, 0.0], [3.0, 1.0]]
OFFSETS = [[0.015, 0.00145, 0.0474], [0.0, 0.02, -0.05], [0.03, -0.01, -0.02], [0.01, 0.0, -0.04], [-0.02, 0.015, -0.03]]
DAMPING, STEP = 0.05, 0.1
# (iters, offsets given, step limit, per-env limit rows): iters = 0 looks at neither the step limit nor the limits
CONFIGS = [(0, off, False, False) for off in (False, True)] + [(it, off, step, rows) for it in (1, 8) for off in (False, True)
                                                                for step in (False, True) for rows in (False, True)]
_CACHE = {}


def _mkey(asset):
    return {"default": "stl", "box": "stl"}.get(asset, asset)


def _model(asset):
    return IK.model_of("cleats" if "cleats" in asset else "default")


def _states():
    if "states" not in _CACHE:
        root, dof, _ = generate_states(NMAX)
        rng = np.random.default_rng(23)
        lo, hi = np.asarray(IK.D.MODEL["dof_lower"]), np.asarray(IK.D.MODEL["dof_upper"])
        _CACHE["states"] = dict(root=root, dof=dof, ball=ball_states(NMAX), delta=rng.uniform(-0.8, 0.8, (NMAX, 18)),
                                qscale=rng.uniform(0.5, 2.0, NMAX),
                                lower=(lo + rng.uniform(0.0, 0.2, (NMAX, 18))).astype(np.float32),
                                upper=(hi - rng.uniform(0.0, 0.2, (NMAX, 18))).astype(np.float32))
    return _CACHE["states"]


def _targets(asset, space, off):
    """fp32 (NMAX, 5, 7): the controlled frames' poses at clip(q + delta), |delta| <= 0.8 rad; computed once and left unchanged"""
    key = ("targets", _mkey(asset), space, off)
    if key not in _CACHE:
        st = _states()
        _CACHE[key] = IK.make_targets(_model(asset), st["root"], st["dof"][:, :, 0], st["delta"], space, OFFSETS if off else None,
                                      asset == "box_cleats", st["qscale"])
    return _CACHE[key]


def _args(asset, space, cfg, mutate=None):
    it, off, step, rows = cfg
    st = _states()
    return dict(model=_model(asset), root=st["root"], dof=st["dof"], targets=_targets(asset, space, off), weights=WEIGHTS,
                offsets=OFFSETS if off else None, damping=DAMPING, max_step=STEP if step else 0.0, iters=it, space=space,
                lower=st["lower"] if rows else None, upper=st["upper"] if rows else None, quirk=asset == "box_cleats", mutate=mutate)


def _bars(model, ref, yard):
    bars = {}
    both = {"q": ref[0], "err": ref[1]}
    for name, (w, ix) in IK.block_slices(model).items():
        bars[name] = 3.0 * yard[name] + 2.0 * float(ulp32(np.abs(both[w][ix]).max()))
    return bars


def _ref(asset, space, cfg):
    """((q, err) in fp64 for NMAX envs, {block: bar}); computed once per key and left unchanged"""
    key = ("ref", _mkey(asset), space, cfg)
    if key not in _CACHE:
        a = _args(asset, space, cfg)
        model = a.pop("model")
        ref = IK.limb_ik_ref(model, **a)
        _CACHE[key] = (ref, _bars(model, ref, IK.yardstick_error(ref, model, **a)))
    return _CACHE[key]


def _ratios(model, got_q, got_e, ref, bars, n):
    both = {"q": (got_q.astype(np.float64), ref[0][:n]), "err": (got_e.astype(np.float64), ref[1][:n])}
    out = {}
    for name, (w, ix) in IK.block_slices(model).items():
        g, r = both[w]
        out[name] = float((np.abs(g[ix] - r[ix]) / bars[name]).max())
    return out


def _prepared(cfg, n, rows=False, root=None, dof=None):
    st = _states()
    sim = _sim(cfg)
    _write_states(sim, st["root"][:n] if root is None else root, st["dof"][:n] if dof is None else dof, st["ball"][:n])
    if rows:
        sim.set_env_params(abi.PARAM_DOF_LOWER, _dev(st["lower"][:n]))
        sim.set_env_params(abi.PARAM_DOF_UPPER, _dev(st["upper"][:n]))
    return sim


def _call(sim, targets, weights=WEIGHTS, offsets=None, damping=DAMPING, max_step=0.0, iters=1, space="env", **kw):
    n = sim.num_envs
    t = targets if isinstance(targets, torch.Tensor) else _dev(targets[:n]).view(n, 5, 7)
    q, e = sim.limb_ik(t, weights, offsets, damping, max_step, iters, space, **kw)
    return _host(q), _host(e)


def _run(sim, asset, space_name, space, cfg, n):
    it, off, step, _ = cfg
    return _call(sim, _targets(asset, space, off), WEIGHTS, OFFSETS if off else None, DAMPING, STEP if step else 0.0, it, space_name)


@pytest.mark.parametrize("task", ["bez_kick", "bez_walk"])
@pytest.mark.parametrize("asset", list(ASSETS4))
def test_known_answer(asset, task):
    """iters 0, 1, 8; ENV and ROOT targets; zero and non-zero offsets; a step limit that bites and none; the model's limits and per-env
    limit rows: q_out and err_out of every env against limb_ik_ref in fp64 on the fp32 inputs"""
    model = _model(asset)
    report = {}
    for n in SIZES:
        for rows in (False, True):
            sim = _prepared(make_cfg(n, task=task, seed=5, **ASSETS4[asset]), n, rows)
            for cfg in CONFIGS:
                if cfg[3] != rows:
                    continue
                for sname, space in SPACES:
                    ref, bars = _ref(asset, space, cfg)
                    q, e = _run(sim, asset, sname, space, cfg, n)
                    assert q.shape == (n, 18) and e.shape == (n, 5, 6) and q.dtype == e.dtype == np.float32
                    for name, v in _ratios(model, q, e, ref, bars, n).items():
                        key = (cfg, sname, name)
                        report[key] = max(report.get(key, 0.0), v)
            sim.close()
    for cfg in CONFIGS:
        for sname, _ in SPACES:
            print("IK_KNOWN_ANSWER %-10s %-8s iters %d offsets %d step %d rows %d %-4s worst error / bar: %s" %
                  ((asset, task) + tuple(int(x) for x in cfg) + (sname, " ".join("%s %.3f" % (b, report[cfg, sname, b]) for b in IK.BLOCKS))))
    cfg = (8, True, True, True)
    st = _states()
    bites = np.abs(_ref(asset, IK.SPACE_ENV, (1, False, True, False))[0][0] - st["dof"][:, :, 0]).max(axis=0)
    assert (np.abs(bites - STEP) < 1e-6).sum() >= 5, "the step limit bites in every chain"
    print("IK_KNOWN_ANSWER bars (iters 8, offsets, step, rows, env):", asset, {k: float("%.3g" % v) for k, v in _ref(asset, IK.SPACE_ENV, cfg)[1].items()})
    assert max(report.values()) <= 1.0, {k: v for k, v in report.items() if v > 1.0}


def test_convergence():
    """starts in the middle 60 % of every joint's range, targets |delta| <= 0.3 rad away (reachable), 30 iterations at the lambda
    tests/test_limb_ik_cpu.py shows to bring the fp64 reference's weighted residual below 1e-4 in every env"""
    model = IK.model_of("default")
    root, q0, T = convergence_inputs(model)
    n = CONV["n"]
    a = (model, root, q0, T, CONV["weights"], None, CONV["damping"], 0.0, CONV["iters"], IK.SPACE_ROOT)
    ref = IK.limb_ik_ref(*a)
    bars = _bars(model, ref, IK.yardstick_error(ref, *a))
    res_ref = IK.weighted_residual(ref[1], CONV["weights"])
    assert res_ref.max() < CONV["bound"]
    dof = np.zeros((n, 18, 2), np.float32)
    dof[:, :, 0] = q0
    sim = _prepared(make_cfg(n, seed=5), n, root=root, dof=dof)
    q, e = _call(sim, T, CONV["weights"], None, CONV["damping"], 0.0, CONV["iters"], "root")
    _, e0 = _call(sim, T, CONV["weights"], iters=0, space="root")
    sim.close()
    W = np.asarray(CONV["weights"])
    room = np.sqrt(3.0 * (W[:, 0] * bars["position"] ** 2 + W[:, 1] * bars["rotation"] ** 2))
    res = IK.weighted_residual(e, CONV["weights"])
    print("IK_CONVERGENCE lambda %g, %d iterations: worst weighted residual GPU %.3e, reference %.3e, at the start %.3e; worst (GPU - reference) / room %.3f"
          % (CONV["damping"], CONV["iters"], res.max(), res_ref.max(), IK.weighted_residual(e0, CONV["weights"]).max(), ((res - res_ref) / room[None, :]).max()))
    assert (res <= res_ref + room[None, :]).all(), float(((res - res_ref) / room[None, :]).max())


@pytest.mark.parametrize("asset", list(ASSETS))
def test_duality_with_the_jacobian_tensor(asset):
    """iters = 1, no step limit, limits out of reach: q_out - q against (J^T W J + lambda^2 I)^-1 J^T W e, J the refreshed Jacobian
    tensor's columns of the chain for its end body turned into the root's axes, e the call's own err_out at iters = 0, solved in fp64"""
    from tests.gpu_util import _J_refs
    st = _states()
    _, barsJ = _J_refs(asset, st["root"], st["dof"], ("J", asset))
    model = _model(asset)
    nb = len(model["body_link"])
    cfg = (1, False, False, False)
    T = _targets(asset, IK.SPACE_ENV, False)
    big = np.full((NMAX, 18), 100.0, np.float32)
    a = _args(asset, IK.SPACE_ENV, cfg)
    a.update(lower=-big, upper=big)
    m = a.pop("model")
    ref = IK.limb_ik_ref(m, **a)
    bars = _bars(m, ref, IK.yardstick_error(ref, m, **a))
    bars0 = _ref(asset, IK.SPACE_ENV, (0, False, False, False))[1]   # e is the call's err_out at iters = 0: that call's bars
    slipped = 0.0
    E0 = IK.quat_to_mat(st["root"][:, 3:7].astype(np.float64), np.float64)
    worst = 0.0
    for n in SIZES:
        sim = _prepared(make_cfg(n, seed=5, **ASSETS[asset]), n)
        sim.set_env_params(abi.PARAM_DOF_LOWER, _dev(-big[:n]))
        sim.set_env_params(abi.PARAM_DOF_UPPER, _dev(big[:n]))
        Jt = sim.dynamics_tensor("jacobian")
        sim.refresh_dynamics_tensors("jacobian")
        J = _host(Jt).astype(np.float64).reshape(n, nb, 6, abi.NUM_GEN)
        _, e0 = _call(sim, T, iters=0)
        q1, _ = _call(sim, T, iters=1)
        sim.close()
        for c, (first, k) in enumerate(IK.chains(model)):
            d0, b = first - 1, IK.end_body(model, c)
            R = IK._T(E0[:n])
            turn = lambda X: np.concatenate([R @ X[:, 0:3], R @ X[:, 3:6]], axis=1)
            aR = np.abs(R)
            Jr, dJ = turn(J[:, b, :, 6 + d0:6 + d0 + k]), np.concatenate([aR @ barsJ[:n, b, 0:3, 6 + d0:6 + d0 + k], aR @ barsJ[:n, b, 3:6, 6 + d0:6 + d0 + k]], axis=1)
            w6 = np.array([WEIGHTS[c][0]] * 3 + [WEIGHTS[c][1]] * 3)
            N = IK._T(Jr) @ (w6[None, :, None] * Jr) + DAMPING ** 2 * np.eye(k)
            e = e0[:, c].astype(np.float64)
            dq = np.linalg.solve(N, IK._T(Jr) @ (w6 * e)[:, :, None])[:, :, 0]
            be = np.array([bars0["position"]] * 3 + [bars0["rotation"]] * 3)
            # first order: d(dq) = N^-1 (dJ^T W e + J^T W de - (dJ^T W J + J^T W dJ) dq)
            rhs = (IK._T(dJ) @ (w6 * np.abs(e))[:, :, None])[:, :, 0] + (IK._T(np.abs(Jr)) @ (w6 * be)[None, :, None])[:, :, 0] \
                + ((IK._T(dJ) @ (w6[None, :, None] * np.abs(Jr)) + IK._T(np.abs(Jr)) @ (w6[None, :, None] * dJ)) @ np.abs(dq)[:, :, None])[:, :, 0]
            tol = (np.abs(np.linalg.inv(N)) @ rhs[:, :, None])[:, :, 0] + bars["q_chain%d" % c]
            got = q1[:, d0:d0 + k].astype(np.float64) - st["dof"][:n, d0:d0 + k, 0].astype(np.float64)
            ratio = np.abs(got - dq) / tol
            worst = max(worst, float(ratio.max()))
            assert (ratio <= 1.0).all(), (asset, n, c, float(ratio.max()))
            assert n < 65 or np.abs(dq).max() > 0.05
            # the same solve with lambda 10 % off: what a slightly wrong solve in the kernel would look like from here
            off = np.linalg.solve(N + (1.1 ** 2 - 1.0) * DAMPING ** 2 * np.eye(k), IK._T(Jr) @ (w6 * e)[:, :, None])[:, :, 0]
            slipped = max(slipped, float((np.abs(got - off) / tol).max()))
    print("IK_VS_JACOBIAN worst |dq - (J^T W J + lambda^2 I)^-1 J^T W e| / tolerance: %s %.3f; with lambda 10 %% off in the fp64 solve: %.1f" % (asset, worst, slipped))
    assert slipped > 1.0, slipped


def test_inactive_chain_and_chain_independence_to_the_bit():
    """a chain with both weights 0 returns the state's q and +0.0f errors whatever its target row holds; all five chains together equal
    each chain alone; a NaN on one active chain stays in that chain; iters = 0 leaves q"""
    n = 65
    st = _states()
    sim = _prepared(make_cfg(n, seed=5, cleats=True), n)
    T = _targets("cleats", IK.SPACE_ENV, True)[:n]
    q0 = st["dof"][:n, :, 0]
    kw = dict(offsets=OFFSETS, max_step=STEP, iters=3)
    qa, ea = _call(sim, T, WEIGHTS, **kw)
    assert np.abs(qa - q0).max() > 0.05
    for c, (d0, d1) in enumerate(abi.IK_CHAIN_DOFS):
        w = [[0.0, 0.0]] * 5
        w[c] = WEIGHTS[c]
        Tn = np.full_like(T, np.nan)                      # the other chains' rows are never looked at
        Tn[:, c] = T[:, c]
        off = [[9.0, 9.0, 9.0]] * 5                       # nor their offsets
        off[c] = OFFSETS[c]
        q1, e1 = _call(sim, Tn, w, off, DAMPING, STEP, 3)
        assert (_bits(q1[:, d0:d1]) == _bits(qa[:, d0:d1])).all() and (_bits(e1[:, c]) == _bits(ea[:, c])).all(), c
        rest = [j for j in range(18) if not d0 <= j < d1]
        assert (_bits(q1[:, rest]) == _bits(q0[:, rest])).all(), c
        assert (_bits(np.delete(e1, c, axis=1)) == 0).all(), c
        # a NaN (position) / an infinity (quaternion) on chain c alone: its outputs are non-finite, the others' bits stay
        for col, bad in ((1, np.nan), (5, np.inf)):
            Tb = T.copy()
            Tb[:, c, col] = bad
            qb, eb = _call(sim, Tb, WEIGHTS, **kw)
            assert not np.isfinite(qb[:, d0:d1]).any() and not np.isfinite(eb[:, c]).any(), (c, col)
            assert (_bits(qb[:, rest]) == _bits(qa[:, rest])).all() and (_bits(np.delete(eb, c, axis=1)) == _bits(np.delete(ea, c, axis=1))).all(), (c, col)
    qz, ez = _call(sim, T, WEIGHTS, OFFSETS, DAMPING, STEP, 0)
    assert (_bits(qz) == _bits(q0)).all() and np.abs(ez).max() > 0.01
    sim.close()


def test_root_space_does_not_read_the_root_pose():
    n = 65
    st = _states()
    T = _targets("default", IK.SPACE_ROOT, False)[:n]
    out = []
    for shift in (False, True):
        root = st["root"][:n].copy()
        if shift:
            root[:, 0:3] += 7.0
            root[:, 3:7] = root[::-1, 3:7]
        sim = _prepared(make_cfg(n, seed=5), n, root=root)
        out.append(_call(sim, T, iters=4, space="root"))
        sim.close()
    assert (_bits(out[0][0]) == _bits(out[1][0])).all() and (_bits(out[0][1]) == _bits(out[1][1])).all()


def test_alignment_and_untouched_state():
    """16-byte aligned buffers and views 4 bytes off give the same bits; the state tensors and an inverse-dynamics result are identical
    before and after the call; results do not depend on N"""
    n = 65
    sim = _prepared(make_cfg(n, seed=5), n, rows=True)
    snap = lambda: [_host(sim.refresh(w)) for w in (abi.TENSOR_ROOT_STATE, abi.TENSOR_DOF_STATE, abi.TENSOR_RIGID_BODY_STATE)] + [_host(sim.inverse_dynamics(None, abi.ID_ALL))]
    before = snap()
    T = _targets("default", IK.SPACE_ENV, True)[:n]
    qa, ea = _call(sim, T, WEIGHTS, OFFSETS, DAMPING, STEP, 5)
    off4 = lambda shape: torch.zeros(torch.Size(shape).numel() + 1, device="cuda:0")[1:].view(shape)
    t, qo, eo = off4((n, 5, 7)), off4((n, 18)), off4((n, 5, 6))
    t.copy_(_dev(T).view(n, 5, 7))
    qb, eb = _call(sim, t, WEIGHTS, OFFSETS, DAMPING, STEP, 5, out=qo, err_out=eo)
    assert (_bits(qa) == _bits(qb)).all() and (_bits(ea) == _bits(eb)).all()
    after = snap()
    for x, y in zip(before, after):
        assert (_bits(x) == _bits(y)).all()
    sim.close()
    sim = _prepared(make_cfg(17, seed=5), 17, rows=True)
    qs, es = _call(sim, T[:17], WEIGHTS, OFFSETS, DAMPING, STEP, 5)
    sim.close()
    assert (_bits(qs) == _bits(qa[:17])).all() and (_bits(es) == _bits(ea[:17])).all()


def test_argument_errors():
    from bez_isaacgym_amd.sim import BezSimError
    import ctypes as C
    n = 4
    sim = _sim(make_cfg(n, seed=5))
    T = torch.zeros(n, 5, 7, device="cuda:0")
    T[:, :, 6] = 1.0
    for kw in (dict(weights=[[1.0, -1.0]] * 5), dict(weights=[[1.0, 1.0]] * 5, damping=0.0), dict(weights=[[1.0, 1.0]] * 5, iters=65),
               dict(weights=[[1.0, 1.0]] * 5, space="local"), dict(weights=[[1.0, 1.0]] * 5, offsets=[[np.inf, 0, 0]] * 5)):
        with pytest.raises(BezSimError):
            sim.limb_ik(T, **kw)
    with pytest.raises(BezSimError):
        sim.limb_ik(T[:, :4], [[1.0, 1.0]] * 5)
    # the library's own checks, past the Python layer
    q, e = torch.zeros(n, 18, device="cuda:0"), torch.zeros(n, 5, 6, device="cuda:0")
    good = abi.ik_params([[1.0, 1.0]] * 5)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    call = lambda p, t=T, qo=q, eo=e: sim.lib.bez_sim_limb_ik(sim.h, None if t is None else ptr(t), C.byref(p), None if qo is None else ptr(qo),
                                                              None if eo is None else ptr(eo), None)
    assert call(good) == 0 and call(good, qo=None) == 0 and call(good, eo=None) == 0
    assert call(good, t=None) == -1 and call(good, qo=None, eo=None) == -1

    def broken(**kw):
        p = abi.ik_params([[1.0, 1.0]] * 5)
        for k, v in kw.items():
            if k == "weight":
                p.weight[2][1] = v
            elif k == "offset":
                p.offset[1][0] = v
            else:
                setattr(p, k, v)
        return p
    for kw in (dict(iters=-1), dict(iters=65), dict(damping=0.0), dict(damping=float("nan")), dict(damping=float("inf")), dict(weight=-1.0),
               dict(weight=float("nan")), dict(offset=float("inf")), dict(space=2)):
        assert call(broken(**kw)) == -1, kw
        assert b"bez_sim_limb_ik" in sim.lib.bez_sim_last_error(sim.h)
    torch.cuda.synchronize()
    sim.close()


SENSITIVITY = (("offset_ignored", "default", (1, True, False, False)), ("weight_ignored", "default", (1, False, False, False)),
               ("step_limit_ignored", "default", (1, False, True, False)), ("limit_rows_ignored", "default", (8, False, False, True)),
               ("quirk_ignored", "box_cleats", (1, False, False, False)))


@pytest.mark.parametrize("mutate,asset,cfg", SENSITIVITY, ids=[s[0] for s in SENSITIVITY])
def test_sensitivity(mutate, asset, cfg):
    """each term, ignored in the reference, puts the GPU's result outside its bar -- a kernel that dropped the term would not pass the
    known-answer test (the quirk: chain 4, the right leg, alone)"""
    n = 65
    model = _model(asset)
    ref, bars = _ref(asset, IK.SPACE_ENV, cfg)
    a = _args(asset, IK.SPACE_ENV, cfg, mutate)
    wrong = IK.limb_ik_ref(a.pop("model"), **a)
    sim = _prepared(make_cfg(n, seed=5, **ASSETS4[asset]), n, cfg[3])
    q, e = _run(sim, asset, "env", IK.SPACE_ENV, cfg, n)
    sim.close()
    right = _ratios(model, q, e, ref, bars, n)
    off = _ratios(model, q, e, wrong, bars, n)
    print("IK_SENSITIVITY %-20s worst error / bar against the reference %.3f, against the reference with the slip %.1f" % (mutate, max(right.values()), max(off.values())))
    assert max(right.values()) <= 1.0
    if mutate == "quirk_ignored":
        assert off["q_chain4"] > 1.0 and all(off["q_chain%d" % c] <= 1.0 for c in range(4)), off
    else:
        assert max(off.values()) > 1.0, off


def test_vec_task_helpers():
    """VecTask.limb_targets holds every limb where it is; ik_offset names the camera's frame on the head chain"""
    from bez_isaacgym_amd.tasks.base.vec_task import VecTask
    n = 17
    st = _states()
    sim = _prepared(make_cfg(n, seed=5), n)

    class Env(VecTask):   # the helpers need the sim and the env count only: no task is set up
        def pre_physics_step(self, actions):
            pass

        def post_physics_step(self):
            pass
    env = Env.__new__(Env)
    env.sim, env.num_environments = sim, n
    T = env.limb_targets()
    assert tuple(T.shape) == (n, 5, 7)
    err = _host(env.limb_pose_error(T))
    q = _host(env.limb_ik(T, [[1.0, 1.0]] * 5, iters=2)[0])   # (the sim's one result buffer: the next call overwrites it)
    c, off = env.ik_offset("/camera")
    assert c == 0 and np.allclose(off, [0.015, 0.00145, 0.0474])
    assert env.ik_offset("/right_foot") == (4, (0.0, 0.0, 0.0))
    with pytest.raises(ValueError):
        env.ik_offset("/left_thigh")
    rb = _host(sim.refresh(abi.TENSOR_RIGID_BODY_STATE)).reshape(n, -1, 13)
    Tc = T.clone()
    Tc[:, 0] = torch.as_tensor(rb[:, env.body_index("/camera"), 0:7]).to(T.device)
    offs = [[0.0, 0.0, 0.0]] * 5
    offs[0] = list(off)
    err_c = _host(env.limb_pose_error(Tc, offsets=offs))
    sim.close()
    # RIGID_BODY_STATE rows are fp32 at up to 100 m (ulp 7.6e-6) and unit quaternions to 1e-7: the error of holding still is rounding
    assert np.abs(err[:, :, 0:3]).max() < 4e-5 and np.abs(err[:, :, 3:6]).max() < 5e-6, (np.abs(err[:, :, 0:3]).max(), np.abs(err[:, :, 3:6]).max())
    assert np.abs(err_c[:, :, 0:3]).max() < 4e-5 and np.abs(err_c[:, :, 3:6]).max() < 5e-6
    assert np.abs(q - st["dof"][:n, :, 0]).max() < 1e-3
