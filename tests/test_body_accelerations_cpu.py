"""CPU: the C ABI declares, lists and exports bez_sim_body_accelerations; its kernel compiles for gfx950 without spills or scratch; and the
reference that pins it on the GPU (tests/body_accel_numpy.acc_ref) is what it says it is -- held to things it was not built from, on the
states of tests/state_sets.generate_states in fp64 -- and notices the mistakes it is there to catch."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from bez_isaacgym_amd import abi
from tests import body_accel_numpy as BA
from tests.state_sets import _expm_skew, generate_states, quat_mat

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "bez_sim.h")).read()
N = 24
G = np.array([0.3, -0.2, -9.81])   # not along an axis: a dropped or permuted component shows
ALL_TERMS = (BA.ACC_UDOT, BA.ACC_VELOCITY, BA.ACC_GRAVITY, BA.ACC_MOTION, BA.ACC_ALL)
SPACES = (BA.SPACE_ENV, BA.SPACE_LOCAL)


def test_abi_declares_lists_and_exports_the_body_acceleration_call():
    """the header declares the function with the issue's signature and the five BEZ_ACC_* values, equal to abi's; sim.EXPORTS and sim.SIGS
    list it; the built library exports it; BEZ_SIM_ABI_VERSION, BEZ_TENSOR_COUNT and the BezDynamicsTensor enum are untouched"""
    assert re.search(r"\bint bez_sim_body_accelerations\(BezSim\* sim, const float\* udot_dev /\* \(N,24\) or NULL \*/, uint32_t terms,\s*"
                     r"int32_t space /\* BEZ_SPACE_ENV \| BEZ_SPACE_LOCAL \*/, float\* out_dev /\* \(N, NB, 6\) \*/, void\* stream\);", HEADER)
    ids = dict((m.group(1), int(m.group(2))) for m in re.finditer(r"#define BEZ_ACC_(\w+)\s+(\d+)u", HEADER))
    assert ids == {"UDOT": abi.ACC_UDOT, "VELOCITY": abi.ACC_VELOCITY, "GRAVITY": abi.ACC_GRAVITY, "MOTION": abi.ACC_MOTION, "ALL": abi.ACC_ALL}
    assert (abi.ACC_UDOT, abi.ACC_VELOCITY, abi.ACC_GRAVITY, abi.ACC_MOTION, abi.ACC_ALL) == (1, 2, 4, 3, 7)
    assert (BA.ACC_UDOT, BA.ACC_VELOCITY, BA.ACC_GRAVITY, BA.ACC_MOTION, BA.ACC_ALL) == (1, 2, 4, 3, 7)
    assert (BA.SPACE_ENV, BA.SPACE_LOCAL) == (abi.SPACE_ENV, abi.SPACE_LOCAL)
    from bez_isaacgym_amd.build import lib_path
    from bez_isaacgym_amd.sim import EXPORTS, SIGS
    assert "bez_sim_body_accelerations" in EXPORTS
    assert SIGS["bez_sim_body_accelerations"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_int32, C.c_void_p, C.c_void_p])
    assert getattr(C.CDLL(lib_path()), "bez_sim_body_accelerations") is not None
    assert int(re.search(r"#define BEZ_SIM_ABI_VERSION (\d+)", HEADER).group(1)) == 5
    body = re.search(r"enum BezDynamicsTensor \{(.*?)\};", HEADER, re.S).group(1)
    assert dict((m.group(1), int(m.group(2))) for m in re.finditer(r"BEZ_DYNAMICS_(\w+) = (\d+)", body)) == {"JACOBIAN": 0, "MASS_MATRIX": 1, "COUNT": 2}
    assert abi.TENSOR_COUNT == 17


def test_the_kernel_of_both_assets_has_no_spills_and_no_scratch(tmp_path):
    from tests.kernel_resources import kernel_resources
    res = kernel_resources(os.path.join(ROOT, "bez_isaacgym_amd", "csrc", "bez_sim.hip"), str(tmp_path))
    mine = {k: v for k, v in res.items() if "body_accelerations_kernel" in k}
    assert len(mine) == 2, sorted(res)
    for name, (vgpr, vspill, sgpr, sspill, scratch, lds) in mine.items():
        print("BODY_ACC_RESOURCES %s: %d VGPRs, %d SGPRs, spills %d / %d, scratch %d B, LDS %d B" % (name, vgpr, sgpr, vspill, sspill, scratch, lds))
        assert vspill == 0 and sspill == 0 and scratch == 0, (name, vspill, sspill, scratch)
        assert 0 < lds <= 64 * 1024


# ---------------------------------------------------------------- the reference

@pytest.fixture(scope="module")
def cases():
    """N states (seams, joint limits, random roots) with exactly unit quaternions, udot of O(10), for the default and the cleats model"""
    root, dof, _ = generate_states(300)
    pick = np.concatenate([np.arange(0, 10), np.arange(40, 300, 17)])[:N]
    root, dof = root[pick].astype(np.float64), dof[pick].astype(np.float64)
    root[:, 3:7] /= np.linalg.norm(root[:, 3:7], axis=1, keepdims=True)
    udot = np.random.default_rng(31).uniform(-10, 10, (N, 24))
    return [dict(model=BA.model_of(asset), asset=asset, root=root, dof=dof, udot=udot) for asset in ("default", "cleats")]


def _ref(c, terms, space=BA.SPACE_ENV, **kw):
    a = dict(root=c["root"], dof=c["dof"], udot=c["udot"], gravity=G)
    a.update(kw)
    return BA.acc_ref(c["model"], a["root"], a["dof"], a["udot"], a["gravity"], terms, space, **{k: v for k, v in kw.items() if k in ("dtype", "mutate")})


def test_the_two_formulations_agree(cases):
    """link-local Pluecker recursion == world axes about the root origin, every term, both spaces, 1e-10 of the block's size"""
    for c in cases:
        for terms in ALL_TERMS:
            for space in SPACES:
                a = _ref(c, terms, space)
                b = BA.acc_ref_world(c["model"], c["root"], c["dof"], c["udot"], G, terms, space)
                assert a.shape == (N, len(c["model"]["body_link"]), 6)
                assert np.abs(a - b).max() <= 1e-10 * max(1.0, np.abs(a).max()), (c["asset"], terms, space, np.abs(a - b).max())


def _velocities(model, root, dof, udot, e, t):
    """J_ref @ u of state e moved for the time t along q + t qd + t^2/2 qdd, R(t) = expm(skew(w t + wdot t^2/2)) R0, u(t) = u + t udot"""
    w, wdot = root[e, 10:13], udot[e, 3:6]
    R = _expm_skew(w * t + wdot * (t * t / 2), 1.0) @ quat_mat(root[e, 3:7])
    q = dof[e, :, 0] + t * dof[e, :, 1] + (t * t / 2) * udot[e, 6:]
    u = np.concatenate([root[e, 7:13], dof[e, :, 1]]) + t * udot[e]
    return BA.J_ref(model, R, q) @ u


def test_motion_is_the_derivative_of_the_body_velocities(cases):
    """ACC_MOTION == d/dt (J u) by a central difference, step h = 2e-6 s, of J_ref @ u (forward kinematics alone) along the trajectory.
    Per env and block the error is taken relative to the block's largest |reference| (some 1e3 m/s^2 or rad/s^2).  Observed: 2.1e-9 at
    h = 2e-6 and 8.5e-9 at h = 4e-6 -- the h^2 law of the truncation h^2 / 6 |d^3 v / dt^3|, the quotient's rounding (1e-16 |v| / h) still
    below it.  The bar is 1e-7 at h = 2e-6, fifty times the observed truncation, and four times that at the doubled step."""
    worst = {}
    for c in cases:
        ref = _ref(c, BA.ACC_MOTION)
        for h in (2e-6, 4e-6):
            for e in range(N):
                fd = (_velocities(c["model"], c["root"], c["dof"], c["udot"], e, h) - _velocities(c["model"], c["root"], c["dof"], c["udot"], e, -h)) / (2 * h)
                for _, sl in BA.BLOCKS:
                    rel = np.abs(fd[:, sl] - ref[e][:, sl]).max() / np.abs(ref[e][:, sl]).max()
                    worst[h] = max(worst.get(h, 0.0), float(rel))
    print("BODY_ACC_FD worst |central difference - acc_ref| / largest |acc_ref| of the block {h: ratio}:", worst)
    assert worst[2e-6] <= 1e-7 and worst[4e-6] <= 4e-7, worst


def test_udot_term_is_the_jacobian_times_udot(cases):
    for c in cases:
        got = _ref(c, BA.ACC_UDOT)
        for e in range(N):
            J = BA.J_ref(c["model"], quat_mat(c["root"][e, 3:7]), c["dof"][e, :, 0])
            want = J @ c["udot"][e]
            assert np.abs(got[e] - want).max() <= 1e-9 * (np.abs(J) @ np.abs(c["udot"][e])).max()


def test_free_fall_reads_zero_and_rest_reads_minus_g(cases):
    """free fall (udot = [g, 0 ...], u = 0, all terms): zero linear rows in both spaces; at rest the gravity term in the body's frame is
    R_b^T (-g) with R_b from forward kinematics alone"""
    for c in cases:
        root, dof = c["root"].copy(), c["dof"].copy()
        root[:, 7:13] = 0
        dof[:, :, 1] = 0
        fall = np.zeros((N, 24))
        fall[:, 0:3] = G
        for space in SPACES:
            out = _ref(c, BA.ACC_ALL, space, root=root, dof=dof, udot=fall)
            assert np.abs(out).max() <= 1e-12, (space, np.abs(out).max())
        rest = _ref(c, BA.ACC_GRAVITY, BA.SPACE_LOCAL, root=root, dof=dof, udot=None)
        assert not rest[:, :, 3:6].any()
        for e in range(N):
            Rb = BA.body_rotations(c["model"], root[e, 3:7], dof[e, :, 0])
            assert np.abs(rest[e, :, 0:3] - np.einsum("bji,j->bi", Rb, -G)).max() <= 1e-12
        env = _ref(c, BA.ACC_GRAVITY, BA.SPACE_ENV, root=root, dof=dof, udot=None)
        assert (env[:, :, 0:3] == -G).all()


def test_terms_add_up_and_dropped_terms_are_exact_zeros(cases):
    for c in cases:
        parts = [_ref(c, t) for t in (BA.ACC_UDOT, BA.ACC_VELOCITY, BA.ACC_GRAVITY)]
        assert np.abs(_ref(c, BA.ACC_ALL) - sum(parts)).max() <= 1e-12 * sum(np.abs(p) for p in parts).max()
        assert np.abs(_ref(c, BA.ACC_MOTION) - parts[0] - parts[1]).max() <= 1e-12 * np.abs(parts[1]).max()
        root, dof = c["root"].copy(), c["dof"].copy()
        root[:, 7:13] = 0
        dof[:, :, 1] = 0
        assert not _ref(c, BA.ACC_UDOT, udot=None).any() and not _ref(c, BA.ACC_GRAVITY, gravity=np.zeros(3)).any()
        assert not _ref(c, BA.ACC_VELOCITY, root=root, dof=dof).any()
        # the torso: udot[0:6] and no bias acceleration; root_lin plays no part (a uniform translation changes no acceleration)
        assert np.abs(parts[0][:, 0] - c["udot"][:, 0:6]).max() <= 1e-13 and np.abs(parts[1][:, 0]).max() <= 1e-12
        moving = c["root"].copy()
        moving[:, 7:10] += 5.0
        assert np.abs(_ref(c, BA.ACC_VELOCITY, root=moving) - parts[1]).max() <= 1e-10


def test_the_reference_is_sensitive(cases):
    """the w x v_p term dropped, cb negated, two DOFs swapped, a fixed body's offset ignored: each moves the reference by more than 100x
    the yardstick's error (the worse of the two fp32 formulations) on the states of generate_states.  The ignored offset shows on the
    camera and, with cleats, on the cleat rows."""
    root, dof, _ = generate_states(64)
    udot = np.random.default_rng(29).uniform(-10, 10, (64, 24)).astype(np.float32)
    perm = np.arange(18); perm[[7, 8]] = perm[[8, 7]]       # knee <-> ankle pitch of the left leg
    for c in cases:
        model = c["model"]
        base = BA.acc_ref(model, root, dof, udot, G, BA.ACC_ALL)
        err32 = BA.yardstick_error(model, root, dof, udot, G, BA.ACC_ALL, BA.SPACE_ENV, base).max()
        assert 0 < err32 < 1e-5 * np.abs(base).max()
        udot_sw = udot.copy(); udot_sw[:, 6:] = udot_sw[:, 6:][:, perm]
        moved = {m: BA.acc_ref(model, root, dof, udot, G, BA.ACC_ALL, mutate=m) for m in ("w_x_vp_dropped", "cb_negated", "offset_ignored")}
        moved["dofs_swapped"] = BA.acc_ref(model, root, dof[:, perm], udot_sw, G, BA.ACC_ALL)
        for what, m in moved.items():
            assert np.abs(m - base).max() > 100 * err32, (c["asset"], what, np.abs(m - base).max(), err32)
        names = model["body_names"]
        off = np.abs(moved["offset_ignored"] - base).max(axis=(0, 2))
        fixed = [b for b, o in enumerate(model["body_offset"]) if any(o)]
        assert names.index("/camera") in fixed and (off[fixed] > 100 * err32).all() and not off[[b for b in range(len(names)) if b not in fixed]].any()
        if c["asset"] == "cleats":
            # the cleat bodies' frames sit AT their foot's origin in this asset (zero body_offset: the URDF puts the offset into the
            # cleats' collision origins), so an ignored offset cannot show on them; what a slip in their link index would change does:
            cleats = [b for b, nm in enumerate(names) if "cleat" in nm]
            assert len(cleats) == 8 and not any(any(model["body_offset"][b]) for b in cleats)
            for b in cleats:
                foot = names.index("/left_foot" if "left" in names[b] else "/right_foot")
                assert model["body_link"][b] == model["body_link"][foot] and (base[:, b] == base[:, foot]).all()
                ankle = names.index("/left_ankle" if "left" in names[b] else "/right_ankle")
                assert np.abs(base[:, b] - base[:, ankle]).max() > 100 * err32   # not the row of the link above
