"""CPU: the references that pin the dynamics tensors (tests/test_gpu_dynamics.py) agree with each other, are what the header says
they are, and notice the mistakes they are there to catch; and the C ABI declares, lists and exports the two entry points."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from bez_isaacgym_amd import abi
from tests import dynamics_numpy as D
from tests import rbd_numpy as R
from tests.sim_cfg import make_cfg
from tests.state_sets import generate_states

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "bez_sim.h")).read()
N = 32
ARMATURE = float(abi.default_config(1).armature)


@pytest.fixture(scope="module")
def states():
    root, dof, _ = generate_states(300)
    pick = np.concatenate([np.arange(0, 12), np.arange(40, 300, 13)])[:N]   # seams, joint limits and random roots alike
    root = root[pick].astype(np.float64)
    # exactly unit quaternions, as in test_fp64_oracle_matches_fd_reference: with the fp32 inputs as they are, |q| - 1 ~ 6e-8 makes
    # quat_to_mat's matrix that far from a rotation, which the routes take differently (1e-7 relative: the GPU bars carry it)
    root[:, 3:7] /= np.linalg.norm(root[:, 3:7], axis=1, keepdims=True)
    return root, dof[pick].astype(np.float64)


@pytest.fixture(scope="module")
def scales():
    s = np.random.default_rng(5).uniform(0.5, 1.5, (N, 19))
    s[: N // 2] = 1.0
    return s


@pytest.fixture(scope="module")
def M_routes(states, scales):
    root, dof = states
    out = {"rnea": [], "jtmj": [], "kane": [], "rnea_cleats": [], "jtmj_cleats": []}
    for e in range(N):
        quat, q, s = root[e, 3:7].astype(np.float64), dof[e, :, 0].astype(np.float64), scales[e]
        out["rnea"].append(D.M_ref_rnea(D.MODEL, quat, q, s, ARMATURE))
        out["jtmj"].append(D.M_ref_jtmj(D.MODEL, quat, q, s, ARMATURE))
        out["kane"].append(D.M_ref_kane(quat, q, s, ARMATURE))
        out["rnea_cleats"].append(D.M_ref_rnea(D.model_of("cleats"), quat, q, s, ARMATURE))
        out["jtmj_cleats"].append(D.M_ref_jtmj(D.model_of("cleats"), quat, q, s, ARMATURE))
    return {k: np.array(v) for k, v in out.items()}


def _rel(a, b):
    """|a - b| / sqrt(M_ii M_jj), worst element"""
    return float(np.max(np.abs(a - b) / D.scale_of(b)))


def test_three_routes_to_M_agree(M_routes):
    """RNEA columns (link-local Pluecker algebra), sum J^T M J (world axes, the model JSON) and Kane's equations (the URDF fixture's 21
    separate bodies) give the same matrix to 1e-10 of sqrt(M_ii M_jj), with and without a mass-scale row; for the cleats model the
    first two (the URDF fixture is the default asset's)"""
    worst = {"rnea~jtmj": _rel(M_routes["rnea"], M_routes["jtmj"]), "kane~jtmj": _rel(M_routes["kane"], M_routes["jtmj"]),
             "cleats rnea~jtmj": _rel(M_routes["rnea_cleats"], M_routes["jtmj_cleats"])}
    print("worst relative difference:", worst)
    assert max(worst.values()) <= 1e-10, worst
    assert _rel(M_routes["jtmj_cleats"], M_routes["jtmj"]) > 1e-3   # (the cleats model is another model)


def test_M_ref_is_symmetric_positive_definite_with_the_documented_blocks(M_routes, scales):
    for key in ("jtmj", "jtmj_cleats"):
        M = M_routes[key]
        assert _rel(M, np.swapaxes(M, 1, 2)) <= 1e-14
        assert np.linalg.eigvalsh(0.5 * (M + np.swapaxes(M, 1, 2))).min() > 0
        mass = np.array([sum(L["mass"] * s for L, s in zip(D.model_of("cleats" if "cleats" in key else "default")["links"], row)) for row in scales])
        np.testing.assert_allclose(M[:, 0:3, 0:3], mass[:, None, None] * np.eye(3), rtol=0, atol=1e-14)


def test_kinetic_energy_is_half_uMu(states, scales, M_routes):
    """1/2 u^T M u = the kinetic energy of tests/rbd_numpy.mechanics + 1/2 armature |qd|^2, u = [root_lin, root_ang, qd]"""
    root, dof = states
    for e in range(N):
        r, q, qd = root[e].astype(np.float64), dof[e, :, 0].astype(np.float64), dof[e, :, 1].astype(np.float64)
        u = np.concatenate([r[7:10], r[10:13], qd])
        ke = R.mechanics(D.scaled_model(D.MODEL, scales[e]), r[0:3], r[3:7], np.concatenate([r[10:13], r[7:10]]), q, qd, np.zeros(3))["KE"]
        want = ke + 0.5 * ARMATURE * qd @ qd
        assert abs(0.5 * u @ M_routes["jtmj"][e] @ u - want) <= 1e-11 * want


def test_J_ref_routes_agree_and_have_the_documented_structure(states):
    """the oracle's unit-velocity rows and the finite-difference FK of the URDF fixture give the same Jacobian; J u is the body rows'
    velocity; the base blocks and the non-ancestor columns are what the header says"""
    from tests.state_sets import oracle_rows
    root, dof = states
    Jo = D.J_ref_oracle(lambda n: make_cfg(n, seed=5), "f64", root, dof, 21)
    Jf = D.J_ref_fd(root, dof)
    assert Jo.shape == Jf.shape == (N, 21, 6, 24)
    # the oracle's rows are fp32 outputs (half an ulp); the central differences with step 1e-5 in fp64 are good to 1e-9
    from tests.state_sets import ulp32
    bad = np.abs(Jo - Jf) > 0.51 * ulp32(Jf) + 1e-9
    assert not bad.any(), (float(np.abs(Jo - Jf).max()), np.argwhere(bad)[:5])
    rows = oracle_rows(make_cfg(N, seed=5), "f64", root, dof)[:, :21].astype(np.float64)
    u = np.concatenate([root[:, 7:13], dof[:, :, 1]], axis=1).astype(np.float64)
    np.testing.assert_allclose(np.einsum("ebrk,ek->ebr", Jo, u), rows[..., 7:13], rtol=0, atol=2e-5)   # (the rows are fp32 outputs)
    eye = np.broadcast_to(np.eye(3), (N, 21, 3, 3))
    np.testing.assert_array_equal(Jo[:, :, 0:3, 0:3], eye)
    np.testing.assert_array_equal(Jo[:, :, 3:6, 3:6], eye)
    np.testing.assert_array_equal(Jo[:, :, 3:6, 0:3], 0 * eye)
    x = rows[:, :, 0:3] - rows[:, :1, 0:3]
    skew = np.zeros((N, 21, 3, 3))
    skew[..., 0, 1], skew[..., 0, 2], skew[..., 1, 0] = -x[..., 2], x[..., 1], x[..., 2]
    skew[..., 1, 2], skew[..., 2, 0], skew[..., 2, 1] = -x[..., 0], -x[..., 1], x[..., 0]
    np.testing.assert_allclose(Jo[:, :, 0:3, 3:6], -skew, rtol=0, atol=2e-5)   # (x from fp32 positions up to 100 m from the origin)
    for b, l in enumerate(D.MODEL["body_link"]):
        anc = set()
        while l > 0:
            anc.add(l)
            l = D.MODEL["links"][l]["parent"]
        for d in range(18):
            col = Jo[:, b, :, 6 + d]
            assert (col == 0).all() if d + 1 not in anc else (np.abs(col[:, 3:6]).max(axis=1) > 0.5).all(), (b, d)


def test_the_references_are_sensitive(states):
    """1 % on one link's mass, and two DOF columns swapped, move M_ref by far more than the GPU bar (which is a few fp32 ulps); the
    swapped columns move J_ref likewise"""
    root, dof = states
    e = 20
    quat, q = root[e, 3:7].astype(np.float64), dof[e, :, 0].astype(np.float64)
    M = D.M_ref_jtmj(D.MODEL, quat, q, None, ARMATURE)
    M32 = D.M_ref_jtmj(D.MODEL, quat, q, None, ARMATURE, dtype=np.float32)
    fp32_err = _rel(M32.astype(np.float64), M)
    assert fp32_err < 1e-5
    for link in range(19):
        def heavier(links, link=link):
            links[link]["mass"] *= 1.01
        moved = _rel(D.M_ref_jtmj(D.MODEL, quat, q, None, ARMATURE, mutate=heavier), M)
        # (links 3 and 11 weigh 0.2 g: 1 % of that is 2e-6 of the joint's inertia -- still 5x what fp32 rounding moves)
        assert moved > (100 if D.MODEL["links"][link]["mass"] > 0.005 else 5) * fp32_err, (link, moved, fp32_err)
    perm = np.arange(24)
    perm[[6 + 7, 6 + 8]] = perm[[6 + 8, 6 + 7]]
    assert _rel(M[np.ix_(perm, perm)], M) > 1e-2
    J = D.J_ref_oracle(lambda n: make_cfg(n, seed=5), "f64", root[e:e + 1], dof[e:e + 1], 21)
    assert np.abs(J[..., perm] - J).max() > 1e-2


def test_abi_declares_lists_and_exports_the_dynamics_entry_points():
    """the header's enum is abi's, both entry points are declared with the issue's signatures, listed in sim.EXPORTS with explicit
    ctypes signatures, and exported by the built library; the BezTensor table is untouched"""
    body = re.search(r"enum BezDynamicsTensor \{(.*?)\};", HEADER, re.S).group(1)
    ids = dict((m.group(1), int(m.group(2))) for m in re.finditer(r"BEZ_DYNAMICS_(\w+) = (\d+)", body))
    assert ids == {"JACOBIAN": abi.DYNAMICS_JACOBIAN, "MASS_MATRIX": abi.DYNAMICS_MASS_MATRIX, "COUNT": abi.DYNAMICS_COUNT}
    assert abi.NUM_GEN == 24 == 6 + abi.NUM_DOFS and abi.TENSOR_COUNT == 17
    assert re.search(r"\bint bez_sim_get_dynamics_tensor\(BezSim\* sim, int which, void\*\* dev_ptr, int64_t shape\[3\], int\* ndim, int\* dtype\);", HEADER)
    assert re.search(r"\bint bez_sim_refresh_dynamics_tensors\(BezSim\* sim, uint32_t which_mask, void\* stream\);", HEADER)
    from bez_isaacgym_amd.build import lib_path
    from bez_isaacgym_amd.sim import EXPORTS, SIGS
    lib = C.CDLL(lib_path())
    for fn in ("bez_sim_get_dynamics_tensor", "bez_sim_refresh_dynamics_tensors"):
        assert fn in EXPORTS and SIGS[fn][0] is C.c_int
        assert getattr(lib, fn) is not None
    assert SIGS["bez_sim_refresh_dynamics_tensors"][1] == [C.c_void_p, C.c_uint32, C.c_void_p]
    assert abi.dynamics_tensor_id("jacobian") == 0 and abi.dynamics_tensor_id("Mass_Matrix") == 1 and abi.dynamics_tensor_id(1) == 1
    for bad in ("coriolis", 2, -1, True, 0.0):
        with pytest.raises(ValueError):
            abi.dynamics_tensor_id(bad)
