"""CPU: the fp64 reference of bez_sim_limb_ik (tests/limb_ik_numpy.py) against finite differences of its own forward kinematics and
against the Jacobian references of tests/dynamics_numpy.py; abi.ik_params' argument checks; the convergence inputs of
tests/test_gpu_limb_ik.py satisfying their condition in the reference alone."""
import math

import numpy as np
import pytest

from bez_isaacgym_amd import abi
from tests import dynamics_numpy as D
from tests import limb_ik_numpy as IK
from tests.limb_ik_inputs import CONV, convergence_inputs
from tests.state_sets import generate_states

W_ALL = [[1.0, 1.0]] * 5


def test_abi_declares_lists_and_exports_the_call():
    """the header declares the call, the struct and the constants as abi mirrors them; sim.SIGS lists it; the built library exports it;
    BEZ_SIM_ABI_VERSION is untouched"""
    import ctypes as C
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "bez_sim.h")).read()
    assert re.search(r"\bint bez_sim_limb_ik\(BezSim\* sim, const float\* targets_dev /\* \(N,5,7\) \*/, const BezIkParams\* params,\s*"
                     r"float\* q_out_dev /\* \(N,18\) or NULL \*/, float\* err_out_dev /\* \(N,5,6\) or NULL \*/, void\* stream\);", header)
    ids = dict((m.group(1), int(m.group(2))) for m in re.finditer(r"#define BEZ_IK_(\w+)\s+(\d+)", header))
    assert ids == {"CHAINS": abi.IK_CHAINS, "SPACE_ENV": abi.IK_SPACE_ENV, "SPACE_ROOT": abi.IK_SPACE_ROOT, "MAX_ITERS": abi.IK_MAX_ITERS}
    assert (IK.SPACE_ENV, IK.SPACE_ROOT, IK.NCH) == (abi.IK_SPACE_ENV, abi.IK_SPACE_ROOT, abi.IK_CHAINS)
    body = re.search(r"typedef struct BezIkParams \{(.*?)\} BezIkParams;", header, re.S).group(1)
    fields = re.findall(r"(float|int32_t)\s+(\w+)((?:\[\w+\])*);", body)
    assert [(t, n, d) for t, n, d in fields] == [("float", "weight", "[BEZ_IK_CHAINS][2]"), ("float", "offset", "[BEZ_IK_CHAINS][3]"),
                                                  ("float", "damping", ""), ("float", "max_step", ""), ("int32_t", "iters", ""), ("int32_t", "space", "")]
    assert [n for n, _ in abi.BezIkParams._fields_] == [n for _, n, _ in fields]
    assert abi.BezIkParams.damping.offset == 4 * 25 and abi.BezIkParams.space.offset == 4 * 28
    from bez_isaacgym_amd.build import lib_path
    from bez_isaacgym_amd.sim import EXPORTS, SIGS
    assert "bez_sim_limb_ik" in EXPORTS
    assert SIGS["bez_sim_limb_ik"] == (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(abi.BezIkParams), C.c_void_p, C.c_void_p, C.c_void_p])
    assert getattr(C.CDLL(lib_path()), "bez_sim_limb_ik") is not None
    assert int(re.search(r"#define BEZ_SIM_ABI_VERSION (\d+)", header).group(1)) == 5


def test_the_kernel_of_both_assets_has_no_spills_and_no_scratch(tmp_path):
    import os
    from tests.kernel_resources import kernel_resources
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = kernel_resources(os.path.join(root, "bez_isaacgym_amd", "csrc", "bez_sim.hip"), str(tmp_path))
    mine = {k: v for k, v in res.items() if "limb_ik_kernel" in k}
    assert len(mine) == 2, sorted(res)
    for name, (vgpr, vspill, sgpr, sspill, scratch, lds) in mine.items():
        print("LIMB_IK_RESOURCES %s: %d VGPRs, %d SGPRs, spills %d / %d, scratch %d B, LDS %d B" % (name, vgpr, sgpr, vspill, sspill, scratch, lds))
        assert vspill == 0 and sspill == 0 and scratch == 0, (name, vspill, sspill, scratch)
        assert 0 < lds <= 64 * 1024


def test_chain_table_matches_the_model_and_abi():
    for asset in ("default", "cleats"):
        m = IK.model_of(asset)
        ch = IK.chains(m)
        assert len(ch) == abi.IK_CHAINS and [(f - 1, f - 1 + k) for f, k in ch] == [tuple(x) for x in abi.IK_CHAIN_DOFS]
        assert [m["body_names"][IK.end_body(m, c)] for c in range(5)] == list(abi.IK_END_BODIES)


def test_reference_jacobian_against_central_differences():
    rng = np.random.default_rng(3)
    m = IK.model_of("default")
    n, h = 40, 1e-6
    q = rng.uniform(D.MODEL["dof_lower"], D.MODEL["dof_upper"], (n, 18))
    off = rng.uniform(-0.05, 0.05, (5, 3)).astype(np.float32)
    for c, (first, k) in enumerate(IK.chains(m)):
        qc = q[:, first - 1:first - 1 + k]
        p, R, A, O = IK.chain_fk(m, c, qc, offset=off[c])
        J = IK.jacobian(p, A, O)
        for j in range(k):
            dq = np.zeros(k); dq[j] = h
            pp, Rp, _, _ = IK.chain_fk(m, c, qc + dq, offset=off[c])
            pm, Rm, _, _ = IK.chain_fk(m, c, qc - dq, offset=off[c])
            np.testing.assert_allclose(J[:, 0:3, j], (pp - pm) / (2 * h), atol=1e-8)
            Wm = (Rp - Rm) / (2 * h) @ IK._T(R)      # skew(angular velocity)
            w = np.stack([Wm[:, 2, 1], Wm[:, 0, 2], Wm[:, 1, 0]], axis=1)
            np.testing.assert_allclose(J[:, 3:6, j], w, atol=1e-8)


def test_pose_error_is_two_sin_half_theta_times_axis():
    rng = np.random.default_rng(5)
    n = 50
    ax = rng.normal(size=(n, 3)); ax /= np.linalg.norm(ax, axis=1, keepdims=True)
    th = rng.uniform(0.0, 3.0, n)
    qd = np.concatenate([ax * np.sin(th / 2)[:, None], np.cos(th / 2)[:, None]], axis=1)
    Rd = IK.quat_to_mat(qd, np.float64)
    eye = np.broadcast_to(np.eye(3), (n, 3, 3))
    e = IK.pose_error(np.ones((n, 3)), Rd, np.zeros((n, 3)), eye, np.float64)
    np.testing.assert_allclose(e[:, 0:3], 1.0)
    np.testing.assert_allclose(e[:, 3:6], 2 * np.sin(th / 2)[:, None] * ax, atol=1e-12)
    np.testing.assert_allclose(IK.pose_error(np.zeros((n, 3)), IK.quat_to_mat(-qd, np.float64), np.zeros((n, 3)), eye, np.float64), e - [1, 1, 1, 0, 0, 0], atol=1e-12)


def test_one_step_against_the_jacobian_reference_columns():
    """one undamped-limit step of the reference equals (J^T W J + lambda^2 I)^-1 J^T W e with J the finite-difference Jacobian reference of
    the dynamics tensors (world axes, URDF fixture), its columns of the chain for the end body turned into the root's axes"""
    root, dof, _ = generate_states(24)
    m = IK.model_of("default")
    J = D.J_ref_fd(root, dof)                                        # (n, nb, 6, 24), world axes
    E0 = IK.quat_to_mat(np.asarray(root, np.float64)[:, 3:7], np.float64)
    rng = np.random.default_rng(9)
    T = IK.make_targets(m, root, dof[:, :, 0], rng.uniform(-0.5, 0.5, (24, 18)), IK.SPACE_ENV)
    w, lam = [[1.0, 0.3]] * 5, 0.05
    big = np.full((24, 18), 100.0)
    q1, _ = IK.limb_ik_ref(m, root, dof, T, w, None, lam, 0.0, 1, IK.SPACE_ENV, -big, big)
    _, e0 = IK.limb_ik_ref(m, root, dof, T, w, None, lam, 0.0, 0, IK.SPACE_ENV)
    W6 = np.diag([1.0, 1.0, 1.0, 0.3, 0.3, 0.3])
    for c, (first, k) in enumerate(IK.chains(m)):
        Jc = J[:, IK.end_body(m, c), :, 6 + first - 1:6 + first - 1 + k]
        Jr = np.concatenate([IK._T(E0) @ Jc[:, 0:3], IK._T(E0) @ Jc[:, 3:6]], axis=1)
        N = IK._T(Jr) @ W6 @ Jr + lam * lam * np.eye(k)
        dq = np.linalg.solve(N, (IK._T(Jr) @ W6 @ e0[:, c, :, None]))[:, :, 0]
        got = q1[:, first - 1:first - 1 + k] - np.asarray(dof, np.float64)[:, first - 1:first - 1 + k, 0]
        # the finite-difference reference is good to about 1e-6 per entry; through a solve with lambda = 0.05 that stays below 1e-3 rad
        np.testing.assert_allclose(got, dq, atol=1e-3)
        assert np.abs(dq).max() > 0.05


def test_ik_params_rejects_each_bad_argument():
    p = abi.ik_params(W_ALL, [[0.0, 0.0, 0.1]] * 5, 0.05, 0.2, 8, "root")
    assert p.iters == 8 and p.space == abi.IK_SPACE_ROOT and abs(p.offset[4][2] - 0.1) < 1e-7 and abs(p.max_step - 0.2) < 1e-7
    assert abi.ik_params(W_ALL).space == abi.IK_SPACE_ENV and abi.ik_params(W_ALL, iters=0).iters == 0
    assert abi.ik_params(W_ALL, iters=abi.IK_MAX_ITERS).iters == abi.IK_MAX_ITERS
    import torch
    assert abi.ik_params(W_ALL, iters=np.int64(8)).iters == 8 and abi.ik_params(W_ALL, iters=np.int32(3)).iters == 3   # any integer type
    assert abi.ik_params(W_ALL, iters=torch.tensor(5)).iters == 5
    import ctypes as C
    assert C.sizeof(abi.BezIkParams) == 4 * (10 + 15 + 4)
    bad_w = [list(r) for r in W_ALL]; bad_w[2][1] = -1.0
    nan_w = [list(r) for r in W_ALL]; nan_w[0][0] = math.nan
    inf_o = [[0.0, 0.0, 0.0] for _ in range(5)]; inf_o[3][1] = math.inf
    for kw in (dict(weights=W_ALL[:4]), dict(weights=None), dict(weights=bad_w), dict(weights=nan_w), dict(weights=W_ALL, offsets=inf_o),
               dict(weights=W_ALL, offsets=[[0.0, 0.0]] * 5), dict(weights=W_ALL, offsets=3), dict(weights=W_ALL, damping=0.0), dict(weights=W_ALL, damping=-0.1),
               dict(weights=W_ALL, damping=math.inf), dict(weights=W_ALL, damping=math.nan), dict(weights=W_ALL, max_step=math.nan),
               dict(weights=W_ALL, iters=-1), dict(weights=W_ALL, iters=abi.IK_MAX_ITERS + 1), dict(weights=W_ALL, iters=1.5),
               dict(weights=W_ALL, iters=True), dict(weights=W_ALL, iters=np.float64(2.0)), dict(weights=W_ALL, iters=np.int64(65)),
dict(weights=W_ALL, space=2), dict(weights=W_ALL, space="local")):
        with pytest.raises(ValueError):
            abi.ik_params(**kw)


def test_fp32_reference_stays_near_fp64():
    """the iteration does not amplify rounding: the np.float32 run of the reference stays near the fp64 run at lambda = 0.05 over 1 and 8
    iterations (the GPU bars are built on this yardstick).  Bound: the normal matrix (entries up to about 2) is rounded to 2^-24 of its
    entries and solved with its smallest eigenvalue >= lambda^2, so a step of up to 0.8 rad is off by up to 2^-24 * 2 / 0.0025 * 0.8 =
    4e-5 rad in the worst (singular) direction; 1e-4 leaves room for the forward kinematics' own rounding, and later iterations correct,
    not add to, the error of earlier ones."""
    root, dof, _ = generate_states(120)
    m = IK.model_of("default")
    rng = np.random.default_rng(2)
    T = IK.make_targets(m, root, dof[:, :, 0], rng.uniform(-0.8, 0.8, (120, 18)), IK.SPACE_ROOT)
    for iters in (1, 8):
        a = (m, root, dof, T, W_ALL, None, 0.05, 0.0, iters, IK.SPACE_ROOT)
        r64 = IK.limb_ik_ref(*a)
        worst = IK.yardstick_error(r64, *a)
        assert max(v for k, v in worst.items() if k.startswith("q_")) < 1e-4, worst


def test_convergence_condition_holds_in_the_reference():
    m = IK.model_of("default")
    root, q, T = convergence_inputs(m)
    qf, err = IK.limb_ik_ref(m, root, q, T, CONV["weights"], None, CONV["damping"], 0.0, CONV["iters"], IK.SPACE_ROOT)
    res = IK.weighted_residual(err, CONV["weights"])
    _, err0 = IK.limb_ik_ref(m, root, q, T, CONV["weights"], None, CONV["damping"], 0.0, 0, IK.SPACE_ROOT)
    print("IK_CONVERGENCE reference: worst weighted residual %.3e (start %.3e), lambda %g" % (res.max(), IK.weighted_residual(err0, CONV["weights"]).max(), CONV["damping"]))
    assert res.max() < CONV["bound"], res.max()
