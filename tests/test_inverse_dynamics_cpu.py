"""CPU: the C ABI declares, lists and exports bez_sim_inverse_dynamics; and the reference that pins it on the GPU
(tests/inverse_dynamics_numpy.id_ref) is what it says it is -- held to identities it was not built from, on the states of
tests/state_sets.generate_states in fp64 -- and notices the mistakes it is there to catch."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from bez_isaacgym_amd import abi
from tests import dynamics_numpy as D
from tests import inverse_dynamics_numpy as ID
from tests import rbd_numpy as R
from tests.state_sets import generate_states

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "bez_sim.h")).read()
N = 24
ARMATURE = float(abi.default_config(1).armature)
G = np.array([0.3, -0.2, -9.81])   # not along an axis: a dropped or permuted component shows
TOL = 1e-9


def test_abi_declares_lists_and_exports_the_inverse_dynamics_call():
    """the header declares the function with the issue's signature and the three BEZ_ID_* values, equal to abi's; sim.EXPORTS and
    sim.SIGS list it; the built library exports it; BEZ_SIM_ABI_VERSION, BEZ_TENSOR_COUNT and the BezDynamicsTensor enum are untouched"""
    assert re.search(r"\bint bez_sim_inverse_dynamics\(BezSim\* sim, const float\* udot_dev, uint32_t terms, float\* out_dev, void\* stream\);", HEADER)
    ids = dict((m.group(1), int(m.group(2))) for m in re.finditer(r"#define BEZ_ID_(\w+)\s+(\d+)u", HEADER))
    assert ids == {"INERTIA": abi.ID_INERTIA, "VELOCITY": abi.ID_VELOCITY, "GRAVITY": abi.ID_GRAVITY, "ALL": abi.ID_ALL}
    assert (abi.ID_INERTIA, abi.ID_VELOCITY, abi.ID_GRAVITY, abi.ID_ALL) == (1, 2, 4, 7)
    assert (ID.ID_INERTIA, ID.ID_VELOCITY, ID.ID_GRAVITY, ID.ID_ALL) == (1, 2, 4, 7)
    from bez_isaacgym_amd.build import lib_path
    from bez_isaacgym_amd.sim import EXPORTS, SIGS
    assert "bez_sim_inverse_dynamics" in EXPORTS
    assert SIGS["bez_sim_inverse_dynamics"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p])
    assert getattr(C.CDLL(lib_path()), "bez_sim_inverse_dynamics") is not None
    assert int(re.search(r"#define BEZ_SIM_ABI_VERSION (\d+)", HEADER).group(1)) == 5
    body = re.search(r"enum BezDynamicsTensor \{(.*?)\};", HEADER, re.S).group(1)
    assert dict((m.group(1), int(m.group(2))) for m in re.finditer(r"BEZ_DYNAMICS_(\w+) = (\d+)", body)) == {"JACOBIAN": 0, "MASS_MATRIX": 1, "COUNT": 2}
    assert (abi.DYNAMICS_JACOBIAN, abi.DYNAMICS_MASS_MATRIX, abi.DYNAMICS_COUNT) == (0, 1, 2) and abi.TENSOR_COUNT == 17


# ---------------------------------------------------------------- the reference

@pytest.fixture(scope="module")
def cases():
    """N states (seams, joint limits, random roots), exactly unit quaternions as in tests/test_dynamics_cpu.py; mass-scale rows (ones for
    the first half); udot of O(10); the default and the cleats model alternate"""
    root, dof, _ = generate_states(300)
    pick = np.concatenate([np.arange(0, 10), np.arange(40, 300, 17)])[:N]
    root, dof = root[pick].astype(np.float64), dof[pick].astype(np.float64)
    root[:, 3:7] /= np.linalg.norm(root[:, 3:7], axis=1, keepdims=True)
    rng = np.random.default_rng(23)
    scale = rng.uniform(0.5, 1.5, (N, 19))
    scale[: N // 2] = 1.0
    udot = rng.uniform(-10, 10, (N, 24))
    out = []
    for e in range(N):
        model = D.model_of("cleats" if e % 2 else "default")
        out.append(dict(model=model, quat=root[e, 3:7], pos=root[e, 0:3], v0=root[e, 7:13], q=dof[e, :, 0], qd=dof[e, :, 1], udot=udot[e],
                        scale=scale[e], u=np.concatenate([root[e, 7:13], dof[e, :, 1]])))
    return out


def _id(c, udot, terms, **kw):
    a = dict(model=c["model"], quat=c["quat"], v0=c["v0"], q=c["q"], qd=c["qd"], udot=udot, gravity=G, mass_scale=c["scale"], armature=ARMATURE,
             terms=terms)
    a.update(kw)
    return ID.id_ref(**a)


def _M(c, quat=None, q=None):
    return D.M_ref_jtmj(c["model"], c["quat"] if quat is None else quat, c["q"] if q is None else q, c["scale"], ARMATURE)


def _row_scale(M, udot):
    """sum_j sqrt(M_ii M_jj) |udot_j|: the size of the terms that make up row i of M udot"""
    return D.scale_of(M) @ np.abs(udot)


def test_the_dtype_generic_rnea_is_rbd_numpys():
    """tests/inverse_dynamics_numpy.rnea in fp64 == tests/rbd_numpy.rnea_floating (the independent inverse dynamics that holds DOF_FORCE)
    to 1e-12 of the result's size, on full states with gravity"""
    root, dof, _ = generate_states(60)
    rng = np.random.default_rng(2)
    for e in range(0, 60, 5):
        quat = root[e, 3:7].astype(np.float64); quat /= np.linalg.norm(quat)
        v0 = np.concatenate([root[e, 10:13], root[e, 7:10]]).astype(np.float64)
        a0, qdd = rng.uniform(-10, 10, 6), rng.uniform(-10, 10, 18)
        q, qd = dof[e, :, 0].astype(np.float64), dof[e, :, 1].astype(np.float64)
        f0, tau = (x[0] for x in ID.rnea(D.MODEL["links"], quat[None], v0[None], a0[None], q[None], qd[None], qdd[None], G[None]))
        g0, gau = R.rnea_floating(D.MODEL, quat, v0, a0, q, qd, qdd, G)
        assert np.abs(f0 - g0).max() <= 1e-12 * np.abs(g0).max() and np.abs(tau - gau).max() <= 1e-12 * np.abs(gau).max()


def test_affine_in_udot_with_the_mass_matrix_as_slope(cases):
    """(a) id_ref(udot) - id_ref(0) == M_ref_jtmj @ udot, and the inertia term alone is that product"""
    for c in cases:
        M = _M(c)
        want, tol = M @ c["udot"], TOL * _row_scale(M, c["udot"])
        assert (np.abs(_id(c, c["udot"], ID.ID_ALL) - _id(c, None, ID.ID_ALL) - want) <= tol + TOL * np.abs(_id(c, None, ID.ID_ALL))).all()
        assert (np.abs(_id(c, c["udot"], ID.ID_INERTIA) - want) <= tol).all()


def test_gravity_power_is_the_rate_of_potential_energy(cases):
    """(b) u . gravity_term == d(PE)/dt = -sum_l m_l g . v_com,l = -g . P with P the linear momentum of tests/rbd_numpy.mechanics"""
    for c in cases:
        mech = R.mechanics(D.scaled_model(c["model"], c["scale"]), c["pos"], c["quat"], np.concatenate([c["v0"][3:6], c["v0"][0:3]]), c["q"], c["qd"], G)
        gt = _id(c, None, ID.ID_GRAVITY)
        assert abs(c["u"] @ gt + G @ mech["P"]) <= TOL * (np.abs(c["u"]) @ np.abs(gt))
        # the force rows: minus the total weight, whatever the pose
        assert np.abs(gt[0:3] + mech["mass"] * G).max() <= TOL * mech["mass"] * np.abs(G).max()


def _advance(c, t):
    """(quat, q) of the state moved along its own velocity for the time t: world-frame angular velocity, xyzw quaternion"""
    w = c["v0"][3:6]
    th = np.linalg.norm(w) * t
    ax = w / np.linalg.norm(w)
    dx, dy, dz, dw = (*(ax * np.sin(th / 2)), np.cos(th / 2))
    x, y, z, s = c["quat"]
    quat = np.array([dw * x + dx * s + dy * z - dz * y, dw * y - dx * z + dy * s + dz * x, dw * z + dx * y - dy * x + dz * s,
                     dw * s - dx * x - dy * y - dz * z])
    return quat, c["q"] + t * c["qd"]


def test_coriolis_power_is_half_u_Mdot_u(cases):
    """(c) u . velocity_term == 1/2 u^T Mdot u (the power balance of M udot + c = forces with d/dt (1/2 u^T M u)), Mdot by central
    differences of M_ref_jtmj along the motion; 1e-5 of sum |u_i| |c_i|: the step 1e-6 s moves angles by 2e-5 rad at most (truncation
    ~ 4e-10 relative) and leaves 1e-16 / 1e-6 = 1e-10 of M in the quotient, against cancellation of up to 1e3 in the sum"""
    dt = 1e-6
    for c in cases:
        Mdot = (_M(c, *_advance(c, dt)) - _M(c, *_advance(c, -dt))) / (2 * dt)
        ct = _id(c, None, ID.ID_VELOCITY)
        assert abs(c["u"] @ ct - 0.5 * c["u"] @ Mdot @ c["u"]) <= 1e-5 * (np.abs(c["u"]) @ np.abs(ct))


def test_free_flight_needs_no_base_wrench(cases):
    """(d) with udot = -M^-1 h (nothing acts on the robot) and with udot = M^-1 ([0; tau] - h) (only its own joints do), rows 0:6 of
    M udot + h vanish -- momentum is conserved -- and rows 6:24 are tau"""
    rng = np.random.default_rng(4)
    for c in cases:
        M, h = _M(c), _id(c, None, ID.ID_VELOCITY | ID.ID_GRAVITY)
        for tau in (np.zeros(18), rng.uniform(-2, 2, 18)):
            rhs = np.concatenate([np.zeros(6), tau])
            udot = np.linalg.solve(M, rhs - h)
            out = _id(c, udot, ID.ID_ALL)
            tol = TOL * (_row_scale(M, udot) + np.abs(h))
            assert (np.abs(out - rhs) <= tol).all(), np.abs(out - rhs).max()


def test_terms_add_up_and_dropped_terms_are_exact_zeros(cases):
    for c in cases:
        parts = [_id(c, c["udot"], t) for t in (ID.ID_INERTIA, ID.ID_VELOCITY, ID.ID_GRAVITY)]
        assert (np.abs(_id(c, c["udot"], ID.ID_ALL) - sum(parts)) <= 1e-12 * sum(np.abs(p) for p in parts)).all()
        assert not _id(c, None, ID.ID_INERTIA).any() and not _id(c, c["udot"], ID.ID_GRAVITY, gravity=np.zeros(3)).any()
        assert not _id(c, c["udot"], ID.ID_VELOCITY, v0=np.zeros(6), qd=np.zeros(18)).any()


def test_the_reference_is_sensitive(cases):
    """(e) one link 1 % heavier, two DOFs swapped, the sign of g flipped: each moves the result by far more (100x) than the error of the
    fp32 yardstick, which is what the GPU bars are made of"""
    for c in cases[:8]:
        base = _id(c, c["udot"], ID.ID_ALL)
        err32 = np.abs(_id(c, c["udot"], ID.ID_ALL, dtype=np.float32).astype(np.float64) - base).max()
        assert 0 < err32 < 1e-4 * np.abs(base).max()
        heavier = c["scale"].copy(); heavier[9] *= 1.01      # a knee
        perm = np.arange(18); perm[[7, 8]] = perm[[8, 7]]       # knee <-> ankle pitch of the left leg
        udot_sw = c["udot"].copy(); udot_sw[6:] = udot_sw[6:][perm]
        swapped = _id(c, udot_sw, ID.ID_ALL, q=c["q"][perm], qd=c["qd"][perm])
        swapped[6:] = swapped[6:][perm]
        for what, moved in (("mass", _id(c, c["udot"], ID.ID_ALL, mass_scale=heavier)), ("swap", swapped), ("gravity", _id(c, c["udot"], ID.ID_ALL, gravity=-G))):
            assert np.abs(moved - base).max() > 100 * err32, (what, np.abs(moved - base).max(), err32)
