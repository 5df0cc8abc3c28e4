"""GPU: bez_sim_generalized_forces (include/bez_sim.h "Generalised forces": sum over bodies of J_b^T w_b, rows [total force; total moment
about the root origin; joint torques]) against the fp64 reference of tests/generalized_forces_numpy.py, against the Jacobian tensor, the
rigid-body velocities, inverse dynamics' gravity term, the step itself, and its own contract to the bit.

Sizes: 1, 15, 16, 17 (the kernel's 16-env tile), 65 (past a wave), 300 (many tiles, ragged last tile).  Assets default / cleats / box in
the kick (ball row) and walk (no ball row) layouts.  No outlier budget anywhere: every element of every env is held to its bar.

  known answer   per block (rows 0:3, 3:6, 6:24): 3x the worst absolute error of gf_ref evaluated in np.float32 against fp64 on the same
                 inputs + 2 fp32 ulps of the block's largest |reference|.
  duality        generalized_forces(at="origin") against J^T w with the refreshed Jacobian tensor, both fp32 on the GPU, the contraction
                 in fp64: 6 NB 2^-23 sum |J| |w| + the Jacobian test's own per-entry bar propagated through |w|.
  power          u . Q against sum_b f . v_b + t . w_b with the refreshed RIGID_BODY_STATE rows: the known-answer bar through |u| + the
                 Jacobian's per-entry bar and the 24-term dot bound (v_b = J_b u) through |w|.

Measured on MI355X: see DESIGN.md 4.3j and profiles/generalized_forces_errors.txt."""
import ctypes as C

import numpy as np
import pytest
import torch

from bez_isaacgym_amd import abi
from tests import dynamics_numpy as D
from tests import generalized_forces_numpy as GF
from tests import inverse_dynamics_numpy as ID
from tests.gpu_util import ASSETS, _bits, _dev, _free, _host, _sim, _write_states
from tests.sim_cfg import make_cfg
from tests.state_sets import ball_states, generate_states, ulp32

pytestmark = pytest.mark.gpu

TILE = 16
SIZES = (1, TILE - 1, TILE, TILE + 1, 65, 300)
NMAX = max(SIZES)
NG = abi.NUM_GEN
KINDS = ("all", "round_robin", "feet")
SPACES = (abi.SPACE_ENV, abi.SPACE_LOCAL)
MODES = (("points", "com"), ("null", "com"), ("null", "origin"))   # (positions given or NULL, at)
_CACHE = {}


def _states():
    if "states" not in _CACHE:
        root, dof, _ = generate_states(NMAX)
        _CACHE["states"] = dict(root=root, dof=dof, ball=ball_states(NMAX))
    return _CACHE["states"]


def _mkey(asset):
    return "cleats" if asset == "cleats" else "stl"


def _load(asset, kind, space):
    """(F, T, X) float32 (NMAX, nb + 1, 3), the last row the ball's; the walk layout takes [:, :nb].  Computed once and left unchanged."""
    key = ("load", _mkey(asset), kind, space)
    if key not in _CACHE:
        st = _states()
        model = GF.model_of(asset)
        _CACHE[key] = GF.loading(kind, model, st["root"], st["dof"], len(model["body_link"]) + 1, space)
    return _CACHE[key]


def _ref(asset, kind, space, mode):
    """(fp64 reference (NMAX, 24), bar (24,)) of an asset's link model for one loading; computed once per key and left unchanged"""
    key = ("ref", _mkey(asset), kind, space, mode)
    if key not in _CACHE:
        st = _states()
        F, T, X = _load(asset, kind, space)
        a = (GF.model_of(asset), st["root"], st["dof"], F, T, X if mode[0] == "points" else None, space, mode[1])
        r64 = GF.gf_ref(*a)
        e32 = GF.yardstick_error(r64, *a)
        bar = np.zeros(NG)
        for k, (_, sl) in enumerate(GF.BLOCKS):
            bar[sl] = 3.0 * e32[k] + 2.0 * float(ulp32(np.abs(r64[:, sl]).max()))
        _CACHE[key] = (r64, bar)
    return _CACHE[key]


def _rows(sim, a, n):
    """the first n envs of a (NMAX, nb + 1, 3) host array as the (n, B, 3) device tensor of the sim's layout"""
    a = a[:n] if sim.has_ball else a[:n, :-1]
    return _dev(a).view(n, sim.num_bodies, 3)


def _prepared(cfg, n):
    st = _states()
    sim = _sim(cfg)
    _write_states(sim, st["root"][:n], st["dof"][:n], st["ball"][:n])
    return sim


def _call(sim, F, T, X=None, space=abi.SPACE_ENV, at="com"):
    return _host(sim.generalized_forces(F, T, X, space, at))


@pytest.mark.parametrize("task", ["bez_kick", "bez_walk"])
@pytest.mark.parametrize("asset", list(ASSETS))
def test_known_answer(asset, task):
    """every body loaded, one body per env round-robin (every body, fixed ones and cleats included, is hit alone) and both feet only; ENV and
    LOCAL; positions given, NULL, and NULL at the origins: every element of every env against gf_ref in fp64 on the fp32 inputs"""
    cfg = lambda n: make_cfg(n, task=task, seed=5, **ASSETS[asset])
    report = {}
    for n in SIZES:
        sim = _prepared(cfg(n), n)
        assert sim.num_bodies == len(GF.model_of(asset)["body_link"]) + (1 if sim.has_ball else 0)
        for kind in KINDS:
            for space in SPACES:
                F, T, X = (_rows(sim, a, n) for a in _load(asset, kind, space))
                for mode in MODES:
                    ref, bar = _ref(asset, kind, space, mode)
                    got = _call(sim, F, T, X if mode[0] == "points" else None, space, mode[1])
                    assert got.shape == (n, NG) and got.dtype == np.float32
                    err = np.abs(got.astype(np.float64) - ref[:n])
                    for name, sl in GF.BLOCKS:
                        key = (kind, "local" if space else "env", mode[0] + "/" + mode[1], name)
                        report[key] = max(report.get(key, 0.0), float((err[:, sl] / bar[sl]).max()))
        sim.close()
    for kind in KINDS:
        for space in ("env", "local"):
            for mode in MODES:
                m = mode[0] + "/" + mode[1]
                print("GF_KNOWN_ANSWER %-7s %-8s %-11s %-5s %-11s worst error / bar: force %.3f moment %.3f joints %.3f" %
                      ((asset, task, kind, space, m) + tuple(report[kind, space, m, name] for name, _ in GF.BLOCKS)))
    print("GF_KNOWN_ANSWER bars (all, env, points):", asset, [float(_ref(asset, "all", 0, MODES[0])[1][sl][0]) for _, sl in GF.BLOCKS])
    assert max(report.values()) <= 1.0, {k: v for k, v in report.items() if v > 1.0}


@pytest.mark.parametrize("asset", list(ASSETS))
def test_duality_with_the_jacobian_tensor_and_power(asset):
    """at="origin", ENV: out[e, c] == sum_{b, r} J[e, b, r, c] w[e, b, r] with the refreshed Jacobian tensor, and u . out == the power of
    the wrenches at the velocities RIGID_BODY_STATE reports"""
    from tests.gpu_util import _J_refs
    st = _states()
    J64, barsJ = _J_refs(asset, st["root"], st["dof"], ("J", asset))
    nb = J64.shape[1]
    cfg = lambda n: make_cfg(n, seed=5, **ASSETS[asset])
    u = np.concatenate([st["root"][:, 7:13], st["dof"][:, :, 1]], axis=1).astype(np.float64)
    worst = {"duality": 0.0, "power": 0.0}
    for n in SIZES:
        sim = _prepared(cfg(n), n)
        Jt = sim.dynamics_tensor("jacobian")
        sim.refresh_dynamics_tensors("jacobian")
        J = _host(Jt).astype(np.float64).reshape(n, nb, 6, NG)
        rb = _host(sim.refresh(abi.TENSOR_RIGID_BODY_STATE)).reshape(n, -1, 13)[:, :nb].astype(np.float64)
        for kind in KINDS:
            Fh, Th, _ = _load(asset, kind, abi.SPACE_ENV)
            got = _call(sim, _rows(sim, Fh, n), _rows(sim, Th, n), None, abi.SPACE_ENV, "origin").astype(np.float64)
            w = np.concatenate([Fh[:n, :nb], Th[:n, :nb]], axis=2).astype(np.float64)
            want = np.einsum("ebrc,ebr->ec", J, w)
            tol = 6 * nb * 2.0 ** -23 * np.einsum("ebrc,ebr->ec", np.abs(J), np.abs(w)) + np.einsum("ebrc,ebr->ec", barsJ[:n], np.abs(w))
            ratio = np.abs(got - want) / np.maximum(tol, 1e-300)
            ratio[(tol == 0) & (got == want)] = 0.0
            worst["duality"] = max(worst["duality"], float(ratio.max()))
            assert (ratio <= 1.0).all(), (asset, n, kind, float(ratio.max()), [tuple(x) for x in np.argwhere(ratio > 1)[:5]])
            # power: the known-answer bar of Q through |u|; v_b = J_b u: the Jacobian's bar and the 24-term dot bound through |w|
            barQ = _ref(asset, kind, abi.SPACE_ENV, ("null", "origin"))[1]
            power = (w[:, :, 0:3] * rb[:, :, 7:10]).sum(axis=(1, 2)) + (w[:, :, 3:6] * rb[:, :, 10:13]).sum(axis=(1, 2))
            bar_v = np.einsum("ebrc,ec->ebr", barsJ[:n] + NG * 2.0 ** -23 * np.abs(J64[:n]), np.abs(u[:n]))
            tolp = np.abs(u[:n]) @ barQ + (np.abs(w) * bar_v).sum(axis=(1, 2))
            rp = np.abs((u[:n] * got).sum(axis=1) - power) / tolp
            worst["power"] = max(worst["power"], float(rp.max()))
            assert (rp <= 1.0).all(), (asset, n, kind, float(rp.max()))
        sim.close()
    print("GF_VS_JACOBIAN worst |Q - J^T w| / tolerance: %s %.3f;  GF_POWER worst |u . Q - power| / tolerance: %.3f" % (asset, worst["duality"], worst["power"]))


@pytest.mark.parametrize("randomized", [False, True], ids=["default_params", "mass_scale_and_gravity_rows"])
@pytest.mark.parametrize("asset", ["default", "box"])
def test_weights_cancel_the_gravity_term(asset, randomized):
    """the weights m_b g at the bodies' centres of mass (NULL positions) + gravity_forces() = inverse_dynamics(None, ID_GRAVITY) cancel
    within the sum of the two calls' known-answer bars.  Body masses: tests/golden/urdf_bodies.json through dynamics_numpy.scaled_bodies
    (the stl assets; the cleats asset has no per-body mass table)."""
    from tests import urdf_independent as U
    st = _states()
    n = 65
    rng = np.random.default_rng(29)
    scale = rng.uniform(0.5, 1.5, (n, 19)).astype(np.float32)
    gravity = (np.array([0.0, 0.0, -9.81]) + rng.uniform(-2, 2, (n, 3))).astype(np.float32)
    cfg = make_cfg(n, seed=5, **ASSETS[asset])
    model = GF.model_of(asset)
    nb = len(model["body_link"])
    sim = _prepared(cfg, n)
    if randomized:
        sim.set_env_params(abi.PARAM_MASS_SCALE, _dev(scale))
        sim.set_env_params(abi.PARAM_GRAVITY, _dev(gravity))
    g = gravity if randomized else np.broadcast_to(np.asarray(list(cfg.gravity), np.float32), (n, 3))
    F = np.zeros((n, nb + 1, 3), np.float32)
    for e in range(n):
        bodies = D.scaled_bodies(U.load_fixture(), scale[e], model["body_link"]) if randomized else U.load_fixture()
        F[e, :nb] = (np.array([B["mass"] for B in bodies])[:, None] * g[e].astype(np.float64)[None, :]).astype(np.float32)
    a = (model, st["root"][:n], st["dof"][:n], F, None, None, abi.SPACE_ENV, "com")
    q64 = GF.gf_ref(*a)
    eq = GF.yardstick_error(q64, *a)
    ia = (model, st["root"][:n], st["dof"][:n], None, g, scale if randomized else None, float(cfg.armature), ID.ID_GRAVITY)
    i64 = ID.id_ref_batch(*ia)
    i32 = ID.id_ref_batch(*ia, dtype=np.float32).astype(np.float64)
    got = _call(sim, _rows(sim, F, n), None).astype(np.float64) + _host(sim.inverse_dynamics(None, abi.ID_GRAVITY)).astype(np.float64)
    sim.close()
    worst = []
    for k, (name, sl) in enumerate(GF.BLOCKS):
        bar = (3.0 * eq[k] + 2.0 * float(ulp32(np.abs(q64[:, sl]).max()))) + (3.0 * float(np.abs(i32[:, sl] - i64[:, sl]).max()) + 2.0 * float(ulp32(np.abs(i64[:, sl]).max())))
        worst.append(float(np.abs(got[:, sl]).max() / bar))
    print("GF_WEIGHTS %s %s worst |Q(weights) + gravity_forces| / bar per block:" % (asset, "randomized" if randomized else "default"), [round(x, 3) for x in worst])
    assert np.abs(q64).max() > 1.0 and max(worst) <= 1.0, worst


@pytest.mark.parametrize("space", ["env", "local"])
@pytest.mark.parametrize("kernel", ["ws8q", "ws8", "lane"])
def test_closure_on_the_step(model, kernel, space, monkeypatch):
    """The set-up of test_equation_of_motion_closes_on_the_step (64 pressed states in free space, one substep): apply_body_forces puts
    wrenches on the torso, a forearm and a foot (ENV with points / LOCAL with points); with udot = (u1 - u0) / h and the pre-step state
    restored, inverse_dynamics(udot, ALL)[:, 0:6] equals generalized_forces(the same tensors)[:, 0:6].  Bar: twice (the worst |rows 0:6| of
    the same identity in the same states with no wrench applied + the known-answer bar of Q for these inputs).
    Joint rows: df_record stores in DOF_FORCE, for a joint that is not speed-limit locked, drive + joint friction + limit and ankle-stop
    torques -- everything the actuator model puts on the joint and nothing of the external wrench -- so ID[6:] - DOF_FORCE = Q[6:] there;
    for a locked joint it stores the constraint's reaction, which is formed from the articulated bias force and is not held to this
    identity here.  Compared: the joints whose ACTUATOR_STATUS carries no lock bit (4 | 8) in the substep."""
    from tests import dof_force_numpy as DF
    from tests.sim_adapter import SimAdapter
    from tests.scenarios import _free_space_cfg, _pressed_state
    n = 64
    monkeypatch.setenv("BEZ_SIM_KERNEL", kernel)
    gmodel = GF.model_of("default")
    names = gmodel["body_names"]
    loaded = [names.index(b) for b in ("/torso", "/left_forearm", "/right_foot")]
    sp = abi.body_force_space(space)

    def run(wrench):
        cfg = _free_space_cfg(n, substeps=1)
        cfg.flags |= abi.FLAG_NO_SELF_COLLISION | abi.FLAG_DOF_FORCE
        sim = SimAdapter(cfg)
        sim.step(np.zeros((n, 18), np.float32))
        acts = DF.inject_pressed(sim, n, model, 21, _pressed_state)
        rs0, ds0 = sim.root_states.copy(), sim.dof_state.copy()
        nbe = sim.sim.num_bodies
        rng = np.random.default_rng(53)
        F, T, X = np.zeros((n, nbe, 3), np.float32), np.zeros((n, nbe, 3), np.float32), rng.uniform(-0.05, 0.05, (n, nbe, 3)).astype(np.float32)
        F[:, loaded] = rng.uniform(-3, 3, (n, 3, 3)); T[:, loaded] = rng.uniform(-0.3, 0.3, (n, 3, 3))
        if sp == abi.SPACE_ENV:
            X += _host(sim.sim.refresh(abi.TENSOR_RIGID_BODY_STATE)).reshape(n, nbe, 13)[:, :, 0:3]
        dev = [_dev(a).view(n, nbe, 3) for a in (F, T, X)]
        if wrench:
            sim.sim.apply_body_forces(dev[0], dev[1], dev[2], sp)
        sim.pre_physics(acts); sim.simulate()
        rs1, ds1 = sim.root_states.copy(), sim.dof_state.copy()
        sim.sim.refresh_actuator_tensors()
        net = _host(sim.sim.actuator_tensor(abi.ACTUATOR_DOF_FORCE)).reshape(n, 18).astype(np.float64)
        status = _host(sim.sim.actuator_tensor(abi.ACTUATOR_STATUS)).reshape(n, 18)
        h = float(cfg.dt) / int(cfg.substeps)
        u0 = np.concatenate([rs0.reshape(n, 2, 13)[:, 0, 7:13], ds0.reshape(n, 18, 2)[:, :, 1]], axis=1).astype(np.float64)
        u1 = np.concatenate([rs1.reshape(n, 2, 13)[:, 0, 7:13], ds1.reshape(n, 18, 2)[:, :, 1]], axis=1).astype(np.float64)
        udot = ((u1 - u0) / h).astype(np.float32)
        sim.set_root_states(rs0.reshape(-1, 13)); sim.set_dof_state(ds0.reshape(-1, 2))
        np.testing.assert_array_equal(sim.dof_state, ds0)
        out = _host(sim.sim.inverse_dynamics(_dev(udot).view(n, NG), abi.ID_ALL)).astype(np.float64)
        Q = _call(sim.sim, dev[0], dev[1], dev[2], sp).astype(np.float64)
        a = (gmodel, rs0.reshape(n, 2, 13)[:, 0], ds0.reshape(n, 18, 2), F, T, X, sp)
        return out, Q, net, (status & 12) == 0, a

    out0, _, net0, free0, _ = run(False)
    out, Q, net, free, a = run(True)
    q64 = GF.gf_ref(*a)
    e32 = GF.yardstick_error(q64, *a)
    barQ = np.zeros(NG)
    for k, (_, sl) in enumerate(GF.BLOCKS):
        barQ[sl] = 3.0 * e32[k] + 2.0 * float(ulp32(np.abs(q64[:, sl]).max()))
    resid0 = [float(np.abs(out0[:, sl]).max()) for sl in (slice(0, 3), slice(3, 6))] + [float(np.abs(out0[:, 6:] - net0)[free0].max())]
    got = [float(np.abs(out[:, sl] - Q[:, sl]).max()) for sl in (slice(0, 3), slice(3, 6))] + [float(np.abs(out[:, 6:] - net - Q[:, 6:])[free].max())]
    bars = [2.0 * (resid0[k] + float(barQ[sl][0])) for k, (_, sl) in enumerate(GF.BLOCKS)]
    print("GF_CLOSURE kernel=%s space=%s |ID - Q| force %.3g (bar %.3g) moment %.3g (bar %.3g), |ID - DOF_FORCE - Q| on %d of %d unlocked joints %.3g (bar %.3g); "
          "no-wrench residuals %s; largest |Q| per block %s" % (kernel, space, got[0], bars[0], got[1], bars[1], int(free.sum()), free.size, got[2], bars[2],
                                                                 [float("%.3g" % r) for r in resid0], [float("%.3g" % np.abs(Q[:, sl]).max()) for _, sl in GF.BLOCKS]))
    assert all(np.abs(Q[:, sl]).max() > 0.1 for _, sl in GF.BLOCKS) and free.sum() > free.size // 2   # not vacuous
    assert np.abs(Q - q64).max() <= barQ.max()
    assert got[0] <= bars[0] and got[1] <= bars[1] and got[2] <= bars[2], (got, bars)


@pytest.mark.parametrize("task", ["bez_kick", "bez_walk"])
@pytest.mark.parametrize("asset", list(ASSETS))
def test_exact_structure(asset, task):
    """every bit-level statement of the header"""
    st = _states()
    n = 65
    sim = _prepared(make_cfg(n, task=task, seed=5, **ASSETS[asset]), n)
    model = GF.model_of(asset)
    names, links, nb = model["body_names"], model["links"], len(model["body_link"])
    nbe = sim.num_bodies
    zero = lambda a: not _bits(a).any()     # +0.0f to the bit
    Z = torch.zeros(n, nbe, 3, device="cuda:0")
    Fa, Ta, Xa = (_rows(sim, a, n) for a in _load(asset, "all", abi.SPACE_ENV))
    for space in SPACES:
        for at in ("com", "origin"):
            assert zero(_call(sim, Z, Z, None, space, at)) and zero(_call(sim, Z, None, None, space, at)) and zero(_call(sim, None, Z, None, space, at))
        assert zero(_call(sim, Z, Z, Xa, space))
    # a wrench on body 0 alone, ENV, its position row bitwise the root position: out[0:6] = [f; t], rows 6:24 +0.0f
    F, T, X = Z.clone(), Z.clone(), Xa.clone()
    F[:, 0], T[:, 0] = Fa[:, 0], Ta[:, 0]
    X[:, 0] = _dev(st["root"][:n, 0:3]).view(n, 3)
    got = _call(sim, F, T, X, abi.SPACE_ENV)
    np.testing.assert_array_equal(_bits(got[:, 0:6]), _bits(np.concatenate([_host(Fa[:, 0]), _host(Ta[:, 0])], axis=1)))
    assert zero(got[:, 6:]) and np.abs(got[:, 0:6]).min() > 0
    # each single-leg loading leaves the other leg's, the arms' and the head's rows +0.0f; so does every single body for the joints
    # that are not on its path
    below = lambda j, l: l == j or (l > 0 and below(j, links[l]["parent"]))     # link l lies on joint j's link or below it
    for space in SPACES:
        Fh, Th, Xh = _load(asset, "all", space)
        for b in [names.index(x) for x in ("/left_foot", "/right_foot", "/left_forearm", "/head", "/camera", "/imu_link", "/left_thigh")] + ([nb - 1] if asset == "cleats" else []):
            F, T = Z.clone(), Z.clone()
            F[:, b], T[:, b] = _rows(sim, Fh, n)[:, b], _rows(sim, Th, n)[:, b]
            got = _call(sim, F, T, _rows(sim, Xh, n), space)
            for j in range(1, len(links)):
                on_path = below(j, model["body_link"][b])
                assert (np.abs(got[:, 5 + j]).max() > 0) if on_path else zero(got[:, 5 + j]), (names[b], j)
            assert np.abs(got[:, 0:6]).min() > 0
    # rows 0:3: the sum of the forces, within 4 ulps of sum |f|
    got = _call(sim, Fa, Ta, Xa, abi.SPACE_ENV)
    Fh = _host(Fa)[:, :nb]
    tot = Fh.astype(np.float64).sum(axis=1)
    assert (np.abs(got[:, 0:3] - tot) <= 4.0 * ulp32(np.abs(Fh).astype(np.float64).sum(axis=1))).all()
    # a zero-force body with a NaN position changes no bit; a NaN ball row changes no bit; a NaN force stays in its env
    Ff, Tf, Xf = (_rows(sim, a, n) for a in _load(asset, "feet", abi.SPACE_ENV))
    want = _call(sim, Ff, Tf, Xf, abi.SPACE_ENV)
    Xn = Xf.clone()
    Xn[:, names.index("/head")] = float("nan"); Xn[:, 0] = float("inf")
    np.testing.assert_array_equal(_bits(_call(sim, Ff, Tf, Xn, abi.SPACE_ENV)), _bits(want))
    for space in SPACES:
        Fs, Ts, Xs = (_rows(sim, a, n) for a in _load(asset, "all", space))
        want_s = _call(sim, Fs, Ts, Xs, space)
        if sim.has_ball:
            Fb, Tb, Xb = Fs.clone(), Ts.clone(), Xs.clone()
            Fb[:, nb] = float("nan"); Tb[:, nb] = float("nan"); Xb[:, nb] = float("nan")
            np.testing.assert_array_equal(_bits(_call(sim, Fb, Tb, Xb, space)), _bits(want_s))
        Fn = Fs.clone()
        Fn[17, names.index("/left_calve"), 1] = float("nan")
        got = _call(sim, Fn, Ts, Xs, space)
        keep = np.arange(n) != 17
        np.testing.assert_array_equal(_bits(got[keep]), _bits(want_s[keep]))
        assert np.isnan(got[17, 0:6]).any() and np.isfinite(got[keep]).all()
    sim.close()


def test_contract():
    """the rc -1 cases with their messages; bez_sim_apply_body_forces keeps refusing the new flag; ten calls allocate nothing; state, inputs
    and pending external wrenches are untouched; a side stream and views one float off 16-byte alignment give the same bits; the Python
    layer checks what it is handed"""
    from bez_isaacgym_amd.sim import BezSimError
    n = 65
    asset = "default"
    sim = _prepared(make_cfg(n, seed=2), n)
    nbe = sim.num_bodies
    F, T, X = (_rows(sim, a, n) for a in _load(asset, "all", abi.SPACE_LOCAL))
    out = torch.zeros(n, NG, device="cuda:0")
    torch.cuda.synchronize()
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    raw = lambda f, t, x, space, o: sim.lib.bez_sim_generalized_forces(sim.h, p(f), p(t), p(x), space, p(o), None)
    for args, word in (((None, None, X, 0, out), b"nothing to map"), ((F, T, X, 2, out), b"BEZ_GF_AT_ORIGIN"), ((F, T, X, 3, out), b"BEZ_GF_AT_ORIGIN"),
                       ((F, T, None, 4, out), b"space"), ((F, T, None, -1, out), b"space"), ((F, T, X, 0, None), b"out_dev")):
        assert raw(*args) == -1, args[3]
        msg = sim.lib.bez_sim_last_error(sim.h)
        assert b"bez_sim_generalized_forces" in msg and word in msg, msg
    assert sim.lib.bez_sim_generalized_forces(None, p(F), p(T), None, 0, p(out), None) == -1
    assert b"bez_sim_generalized_forces" in sim.lib.bez_sim_last_error(None)
    assert not out.any()
    # the apply call: any value other than 0 and 1 is refused, exactly as before
    for space in (2, 3):
        assert sim.lib.bez_sim_apply_body_forces(sim.h, p(F), p(T), None, space, None) == -1
        assert b"bez_sim_apply_body_forces" in sim.lib.bez_sim_last_error(sim.h)
    # pending external wrenches: applied, then left alone by the query -- the step after it moves as the step of a sim that never queried
    snap = lambda s: [_host(s.refresh(w)) for w in (abi.TENSOR_ROOT_STATE, abi.TENSOR_DOF_STATE, abi.TENSOR_DOF_TARGET)]
    twin = _prepared(make_cfg(n, seed=2), n)
    acts = torch.zeros(n * 18, device="cuda:0")
    for s in (sim, twin):
        s.apply_body_forces(F, T, X, abi.SPACE_LOCAL)
    state = snap(sim)
    inputs = [_host(t) for t in (F, T, X)]
    want = _call(sim, F, T, X, abi.SPACE_LOCAL)
    before = _free()
    for k in range(10):
        sim.generalized_forces(F if k % 3 else None, T, X if k % 2 else None, SPACES[k % 2], "com" if k % 2 else "origin", out if k % 4 else None)
    assert _free() == before
    for a, b in zip(state, snap(sim)):
        np.testing.assert_array_equal(_bits(a), _bits(b))
    for a, t in zip(inputs, (F, T, X)):
        np.testing.assert_array_equal(_bits(a), _bits(_host(t)))
    assert raw(F, T, X, abi.SPACE_LOCAL, out) == 0
    np.testing.assert_array_equal(_bits(_host(out)), _bits(want))
    out.zero_()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        sim.generalized_forces(F, T, X, "local", out=out)
    np.testing.assert_array_equal(_bits(_host(out)), _bits(want))
    assert np.abs(want).max() > 10
    # views that are contiguous but only 4-byte aligned take the kernel's scalar paths: same bits, and not a float outside the view
    pad = torch.full((n * NG + 2,), -7.0, device="cuda:0")
    pad_o = pad[1:-1].view(n, NG)
    off = []
    for t in (F, T, X):
        buf = torch.zeros(n * nbe * 3 + 1, device="cuda:0")
        buf[1:] = t.reshape(-1)
        off.append(buf[1:].view(n, nbe, 3))
    sim.generalized_forces(off[0], off[1], off[2], abi.SPACE_LOCAL, out=pad_o)
    np.testing.assert_array_equal(_bits(_host(pad_o)), _bits(want))
    assert _host(pad)[0] == -7.0 and _host(pad)[-1] == -7.0
    np.testing.assert_array_equal(_bits(_call(sim, F.view(n * nbe, 3), T.view(n * nbe, 3), X.view(n * nbe, 3), abi.SPACE_LOCAL)), _bits(want))
    for s in (sim, twin):
        s.step(acts)
    for a, b in zip(snap(sim), snap(twin)):
        np.testing.assert_array_equal(_bits(a), _bits(b))
    for bad in (dict(forces=F[:, :-1]), dict(forces=F.double()), dict(forces=F.cpu()), dict(forces=F.transpose(0, 1).contiguous().transpose(0, 1)),
                dict(forces=_host(F)), dict(forces=None, torques=None), dict(forces=F, positions=X, at="origin"), dict(forces=F, out=out[:-1]),
                dict(forces=F, out=out.reshape(-1)), dict(forces=F, torques=T[:-1])):
        with pytest.raises(BezSimError):
            sim.generalized_forces(**bad)
    for bad in (dict(space="world"), dict(at="foot"), dict(space=2)):
        with pytest.raises(ValueError):
            sim.generalized_forces(F, T, **bad)
    sim.close(); twin.close()


def test_call_captures_into_a_graph():
    """captured once, replayed after the state and the inputs changed in place, it gives what a direct call gives"""
    n = 65
    st = _states()
    sim = _sim(make_cfg(n, seed=2))
    Fh, Th, Xh = _load("default", "all", abi.SPACE_ENV)
    F, T, X = (torch.zeros(n, sim.num_bodies, 3, device="cuda:0") for _ in range(3))
    out = torch.zeros(n, NG, device="cuda:0")
    sim.generalized_forces(F, T, X, abi.SPACE_ENV, out=out)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        sim.generalized_forces(F, T, X, abi.SPACE_ENV, out=out)
    _write_states(sim, st["root"][:n], st["dof"][:n], st["ball"][:n])
    for t, h in ((F, Fh), (T, Th), (X, Xh)):
        t.copy_(_rows(sim, h, n))
    g.replay()
    got = _host(out)
    direct = _call(sim, F, T, X, abi.SPACE_ENV)
    np.testing.assert_array_equal(_bits(got), _bits(direct))
    assert np.abs(got).max() > 10
    sim.close()


def test_vec_task_methods():
    """VecTask.generalized_forces passes through; body_wrench_forces is the raw call with one loaded row at the body's origin, and leaves
    its two buffers zero"""
    from bez_isaacgym_amd.utils.config import load_config
    from bez_isaacgym_amd.utils.rlgames_utils import get_rlgames_env_creator
    n = 64
    cfg = load_config(["task=bez_kick", "num_envs=%d" % n, "headless=True"])
    env = get_rlgames_env_creator(cfg["task"], "bez_kick", "cuda:0", "cuda:0", 0, True)()
    env.step(torch.rand(n, 18, device=env.device) * 2 - 1)
    nbe = env.sim.num_bodies
    names = GF.model_of("default")["body_names"]
    out = torch.zeros(n, NG, device=env.device)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    direct = lambda f, t, x, space: env.sim.lib.bez_sim_generalized_forces(env.sim.h, p(f), p(t), p(x), space, p(out), stream)
    F, T, X = torch.rand(n, nbe, 3, device=env.device) * 20 - 10, torch.rand(n, nbe, 3, device=env.device) * 2 - 1, torch.rand(n, nbe, 3, device=env.device) * 0.1
    for kw, args in ((dict(forces=F, torques=T, positions=X, space="local"), (F, T, X, 1)), (dict(forces=F), (F, None, None, 0)),
                     (dict(torques=T, space="local", at="origin"), (None, T, None, 3))):
        assert direct(*args) == 0
        t = env.generalized_forces(**kw)
        assert tuple(t.shape) == (n, NG) and t.dtype == torch.float32
        np.testing.assert_array_equal(_bits(_host(t)), _bits(_host(out)))
    f, t = F[:, 0].contiguous(), T[:, 0].contiguous()
    for body in ("/left_foot", "/right_forearm", "/camera"):
        for kw, space in ((dict(force=f, torque=t), 2), (dict(force=f, space="local"), 3), (dict(torque=t, at="com"), 0)):
            Fo, To = torch.zeros_like(F), torch.zeros_like(T)
            if "force" in kw:
                Fo[:, names.index(body)] = f
            if "torque" in kw:
                To[:, names.index(body)] = t
            assert direct(Fo, To, None, space) == 0
            got = env.body_wrench_forces(body, **kw)
            np.testing.assert_array_equal(_bits(_host(got)), _bits(_host(out)))
            assert np.abs(_host(got)).max() > 0.1
    assert not any(b.any() for b in env._wrench_rows)
    with pytest.raises(ValueError):
        env.body_wrench_forces("/no_such_body", force=f)
    with pytest.raises(ValueError):
        env.body_wrench_forces("/left_foot")
