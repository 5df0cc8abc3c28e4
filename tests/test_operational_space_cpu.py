"""CPU: the C ABI declares, lists and exports bez_sim_operational_space; the reference that pins it on the GPU
(tests/operational_space_numpy.op_space_ref) agrees with the independent finite-difference Jacobian, gives a symmetric PSD W of rank <= 24
with Lambda_c W_cc = I, equals the block-arrow elimination the kernel uses, stays well-posed on the states of the GPU tests, and notices
the mistakes it is there to catch; abi.op_space_params rejects what it must."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from bez_isaacgym_amd import abi
from tests import dynamics_numpy as D
from tests import forward_dynamics_numpy as FD
from tests import limb_ik_numpy as IK
from tests import operational_space_numpy as OS
from tests.state_sets import generate_states

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "bez_sim.h")).read()
ARMATURE = float(abi.default_config(1).armature)
OFFSETS = [[0, 0, .03], [0, 0, -.05], [.02, 0, -.01], [0, 0, -.05], [.02, 0, -.01]]
N = 12


def test_abi_declares_lists_and_exports_the_operational_space_call():
    """the header declares the function and the struct with the issue's signature, in a section between "Forward dynamics:" and
    "Centroidal dynamics:"; sim.EXPORTS and sim.SIGS list it; the built library exports it; BEZ_SIM_ABI_VERSION is untouched"""
    assert re.search(r"typedef struct BezOpSpaceParams \{\s*float offset\[BEZ_IK_CHAINS\]\[3\];[^}]*?uint32_t mode;[^}]*\} BezOpSpaceParams;", HEADER)
    note = r"\s*/\*[^*]*\*/,\s*"
    assert re.search(r"\bint bez_sim_operational_space\(BezSim\* sim, const BezOpSpaceParams\* params,\s*float\* jac_dev" + note + r"float\* jminv_dev" + note +
                     r"float\* w_dev" + note + r"float\* lambda_dev" + note + r"void\* stream\);", HEADER)
    assert HEADER.index("Inverse dynamics:") < HEADER.index("Forward dynamics:") < HEADER.index("Operational space:") < HEADER.index("Centroidal dynamics:")
    assert int(re.search(r"#define BEZ_SIM_ABI_VERSION (\d+)", HEADER).group(1)) == abi.ABI_VERSION == 5
    from bez_isaacgym_amd.build import lib_path
    from bez_isaacgym_amd.sim import EXPORTS, SIGS, BezSim
    assert "bez_sim_operational_space" in EXPORTS
    assert SIGS["bez_sim_operational_space"] == (C.c_int, [C.c_void_p, C.POINTER(abi.BezOpSpaceParams)] + [C.c_void_p] * 5)
    assert getattr(C.CDLL(lib_path()), "bez_sim_operational_space") is not None
    assert callable(BezSim.operational_space)
    assert C.sizeof(abi.BezOpSpaceParams) == 4 * (3 * abi.IK_CHAINS + 1)
    assert OS.NCH == abi.IK_CHAINS and OS.NG == abi.NUM_GEN
    for name in ("operational_space", "end_effector_jacobian", "delassus_matrix", "operational_space_inertia", "dynamically_consistent_inverse"):
        from bez_isaacgym_amd.tasks.base.vec_task import VecTask
        assert callable(getattr(VecTask, name))


@pytest.fixture(scope="module")
def cases():
    """per link model: N states (seams, joint limits, random roots) with exactly unit quaternions, mass-scale rows (ones for the first
    half), and the fp64 reference with the issue's offsets"""
    root, dof, _ = generate_states(300)
    out = {}
    for k, asset in enumerate(("default", "cleats")):
        pick = (np.concatenate([np.arange(0, 10), np.arange(40, 300, 17)])[:2 * N])[k::2]
        r, d = root[pick].astype(np.float64), dof[pick].astype(np.float64)
        r[:, 3:7] /= np.linalg.norm(r[:, 3:7], axis=1, keepdims=True)
        scale = np.random.default_rng(31 + k).uniform(0.5, 1.5, (N, 19))
        scale[: N // 2] = 1.0
        model = D.model_of(asset)
        a = dict(model=model, root=r, dof=d, offsets=OFFSETS, scale=scale, armature=ARMATURE, quirk=asset == "cleats")
        out[asset] = dict(a, ref=OS.op_space_ref(**a))
    return out


def _args(c, **kw):
    a = {k: c[k] for k in ("model", "root", "dof", "offsets", "scale", "armature", "quirk")}
    a.update(kw)
    return a


def test_the_reference_jacobian_is_the_finite_difference_one():
    """at offset 0 J_E equals the rows of the end bodies in the finite-difference Jacobian of the URDF fixture (default asset), to that
    reference's own accuracy (1e-6 per entry at |x| <= 100 m)"""
    root, dof, _ = generate_states(12)
    m = D.model_of("default")
    Jf = D.J_ref_fd(root, dof)
    J = OS.frame_jacobians(m, root, dof)
    for c in range(OS.NCH):
        np.testing.assert_allclose(J[:, c], Jf[:, IK.end_body(m, c)], atol=2e-6)
    assert np.abs(J).max() > 0.1
    assert [m["body_names"][IK.end_body(m, c)] for c in range(5)] == list(abi.IK_END_BODIES)


def test_the_reference_is_right(cases):
    """W is symmetric, PSD to 1e-10 of its largest entry and of rank <= 24; Lambda_c W_cc = I to 1e-9; block_arrow_solve on the 30 columns
    equals the dense solve to 1e-10 of the largest entry; the fixed base gives block-diagonal W and zero base columns"""
    for c in cases.values():
        ref = c["ref"]
        W, big = ref["w"], np.abs(ref["w"]).max()
        assert np.abs(W - np.swapaxes(W, 1, 2)).max() <= 1e-12 * big
        ev = np.linalg.eigvalsh(0.5 * (W + np.swapaxes(W, 1, 2)))
        assert ev.min() >= -1e-10 * big
        assert (np.linalg.matrix_rank(W, tol=1e-9 * big) <= 24).all()
        eye = np.eye(6)
        for k in range(OS.NCH):
            assert np.abs(ref["lambda"][:, k] @ W[:, 6 * k:6 * k + 6, 6 * k:6 * k + 6] - eye).max() <= 1e-9
        M = OS.mass_matrices(c["model"], c["root"], c["dof"], c["scale"], ARMATURE, quirk=c["quirk"])
        JE = ref["jac"].reshape(N, OS.NF, OS.NG)
        for e in range(N):
            T = np.stack([FD.block_arrow_solve(M[e], JE[e, k]) for k in range(OS.NF)], axis=1)
            assert np.abs(T - ref["minvjt"][e]).max() <= 1e-10 * np.abs(ref["minvjt"][e]).max()
        np.testing.assert_allclose(ref["jminv"].reshape(N, OS.NF, OS.NG), np.swapaxes(ref["minvjt"], 1, 2))
        fx = OS.op_space_ref(**_args(c, fixed_base=True, M=M))
        assert fx["lambda"] is None and not fx["jminv"][..., 0:6].any()
        off = ~np.kron(np.eye(OS.NCH, dtype=bool), np.ones((6, 6), bool))
        assert not fx["w"][:, off].any() and np.abs(fx["w"]).max() > 1
        np.testing.assert_array_equal(fx["jac"], ref["jac"])


def test_the_inputs_keep_the_reference_well_posed():
    """a condition on the inputs, not a measurement: on all 300 states of the GPU tests, for both link models, with and without the
    mass-scale rows, at offset zero and at the issue's offsets, cond(W_cc) <= 1e5 for every chain with a floating base"""
    from tests.gpu_util import _states
    st = _states()
    worst = 0.0
    for asset in ("default", "cleats"):
        model = D.model_of(asset)
        for scale in (None, st["scale"]):
            M = OS.mass_matrices(model, st["root"], st["dof"], scale, ARMATURE)
            for off in (None, OFFSETS):
                W = OS.op_space_ref(model, st["root"], st["dof"], off, scale, ARMATURE, M=M, want_lambda=False)["w"]
                cond = np.stack([np.linalg.cond(W[:, 6 * c:6 * c + 6, 6 * c:6 * c + 6]) for c in range(OS.NCH)], axis=1)
                print("OS_COND", asset, "scaled" if scale is not None else "default", "offsets" if off else "zero", "min %.3g max %.3g" % (cond.min(), cond.max()))
                worst = max(worst, float(cond.max()))
    assert worst <= 1e5, worst


def test_the_reference_is_sensitive(cases):
    """each planted slip moves every output it touches by more than the bar the GPU is held to (per class: 3x the worst error of the fp32
    evaluation + 2 fp32 ulps of the largest |reference|), on the envs that carry a mass-scale row; the cleats model stands for box + cleats"""
    touched = {"offset_ignored": OS.OUTPUTS, "linear_rows_at_body_origin": OS.OUTPUTS, "quirk_ignored": OS.OUTPUTS,
               "armature_dropped": OS.OUTPUTS[1:], "mass_scale_dropped": OS.OUTPUTS[1:]}
    assert set(touched) == set(OS.MUTATIONS)
    half = slice(N // 2, N)
    for asset, c in cases.items():
        bars = OS.class_bars(c["ref"], OS.op_space_ref(**_args(c, dtype=np.float32)))
        ref = {k: v[half] for k, v in c["ref"].items()}
        for mut, outs in touched.items():
            if mut == "quirk_ignored" and not c["quirk"]:
                continue
            moved = OS.op_space_ref(**_args(c, mutate=mut))
            ratio = OS.class_ratios({k: v[half] for k, v in moved.items()}, ref, bars)
            for o in outs:
                best = max(v for k, v in ratio.items() if OS.classes()[k][0] == o)
                print("OS_SENSITIVE", asset, mut, o, "shift / bar = %.3g" % best)
                assert best > 1.0, (asset, mut, o, ratio)


def test_op_space_params_rejects_each_bad_argument():
    p = abi.op_space_params(OFFSETS, True)
    assert p.mode == abi.FD_FIXED_BASE and abs(p.offset[2][0] - 0.02) < 1e-8 and abs(p.offset[4][2] + 0.01) < 1e-8
    p = abi.op_space_params()
    assert p.mode == 0 and not any(p.offset[c][k] for c in range(5) for k in range(3))
    assert abi.op_space_params(np.asarray(OFFSETS, np.float32), False).offset[0][2] == np.float32(0.03)
    nan = [list(r) for r in OFFSETS]; nan[3][1] = float("nan")
    inf = [list(r) for r in OFFSETS]; inf[0][0] = float("inf")
    for bad in (OFFSETS[:4], [r[:2] for r in OFFSETS], [OFFSETS], 1.0, nan, inf, np.zeros((3, 5))):
        with pytest.raises(ValueError):
            abi.op_space_params(bad)
    with pytest.raises(ValueError):
        abi.op_space_params(None, "yes")
