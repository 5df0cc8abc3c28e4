"""CPU: the C ABI declares, lists and exports bez_sim_forward_dynamics; and the reference that pins it on the GPU
(tests/forward_dynamics_numpy.fd_ref_batch) inverts the inverse dynamics it is held against, rests on a mass matrix with the block-arrow
structure the kernel relies on, and notices the mistakes it is there to catch."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from bez_isaacgym_amd import abi
from tests import dynamics_numpy as D
from tests import forward_dynamics_numpy as FD
from tests import inverse_dynamics_numpy as ID
from tests.state_sets import generate_states, ulp32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "bez_sim.h")).read()
N = 12                                  # per asset
ARMATURE = float(abi.default_config(1).armature)
G = np.array([0.3, -0.2, -9.81])        # not along an axis: a dropped or permuted component shows
BIASES = (FD.BIAS_ALL, ID.ID_VELOCITY, ID.ID_GRAVITY, 0)


def test_abi_declares_lists_and_exports_the_forward_dynamics_call():
    """the header declares the function with the issue's signature and BEZ_FD_FIXED_BASE, equal to abi's; sim.EXPORTS and sim.SIGS list
    it; the built library exports it; BEZ_SIM_ABI_VERSION is untouched"""
    assert re.search(r"\bint bez_sim_forward_dynamics\(BezSim\* sim, const float\* force_dev, uint32_t bias, uint32_t mode, float\* out_dev, "
                     r"void\* stream\);", HEADER)
    assert int(re.search(r"#define BEZ_FD_FIXED_BASE\s+(\d+)u", HEADER).group(1)) == abi.FD_FIXED_BASE == 1
    assert HEADER.index("Inverse dynamics:") < HEADER.index("Forward dynamics:") < HEADER.index("Centroidal dynamics:")
    from bez_isaacgym_amd.build import lib_path
    from bez_isaacgym_amd.sim import EXPORTS, SIGS, BezSim
    assert "bez_sim_forward_dynamics" in EXPORTS
    assert SIGS["bez_sim_forward_dynamics"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p])
    assert getattr(C.CDLL(lib_path()), "bez_sim_forward_dynamics") is not None
    assert callable(BezSim.forward_dynamics)
    assert int(re.search(r"#define BEZ_SIM_ABI_VERSION (\d+)", HEADER).group(1)) == 5
    assert (FD.ID_VELOCITY, FD.ID_GRAVITY, FD.BIAS_ALL) == (abi.ID_VELOCITY, abi.ID_GRAVITY, abi.ID_VELOCITY | abi.ID_GRAVITY)


@pytest.fixture(scope="module")
def cases():
    """per asset: N states (seams, joint limits, random roots) with exactly unit quaternions, mass-scale rows (ones for the first half),
    forces of +-5 N and +-0.5 N m, and M of every state in fp64"""
    root, dof, _ = generate_states(300)
    out = {}
    for k, asset in enumerate(("default", "cleats")):
        pick = (np.concatenate([np.arange(0, 10), np.arange(40, 300, 17)])[:2 * N])[k::2]
        r, d = root[pick].astype(np.float64), dof[pick].astype(np.float64)
        r[:, 3:7] /= np.linalg.norm(r[:, 3:7], axis=1, keepdims=True)
        rng = np.random.default_rng(31 + k)
        scale = rng.uniform(0.5, 1.5, (N, 19))
        scale[: N // 2] = 1.0
        force = rng.uniform(-1, 1, (N, 24)) * np.where(np.arange(24) < 3, 5.0, 0.5)
        model = D.model_of(asset)
        out[asset] = dict(model=model, root=r, dof=d, scale=scale, force=force, M=FD.M_batch(model, r, d, scale, ARMATURE))
    return out


def _fd(c, bias, fixed, dtype=np.float64, **kw):
    a = dict(model=c["model"], root=c["root"], dof=c["dof"], force=c["force"], g=G, scale=c["scale"], armature=ARMATURE, bias=bias,
             fixed_base=fixed, dtype=dtype)
    a.update(kw)
    return FD.fd_ref_batch(**a)


def test_the_reference_inverts_the_inverse_dynamics(cases):
    """id_ref(fd_ref(f), ID_INERTIA | bias) == f to 1e-9 of the row's sum_j |M_ij| |x_j| in fp64; with the root held, on rows 6:24"""
    for c in cases.values():
        for bias in BIASES:
            for fixed in (False, True):
                x = _fd(c, bias, fixed, M=c["M"])
                back = ID.id_ref_batch(c["model"], c["root"], c["dof"], x, G, c["scale"], ARMATURE, ID.ID_INERTIA | bias)
                tol = 1e-9 * np.einsum("eij,ej->ei", np.abs(c["M"]), np.abs(x))
                lo = 6 if fixed else 0
                assert (np.abs(back - c["force"])[:, lo:] <= tol[:, lo:]).all(), (bias, fixed, float((np.abs(back - c["force"]) / tol)[:, lo:].max()))
                if fixed:
                    assert not x[:, 0:6].any()


def test_the_mass_matrix_is_a_block_arrow(cases):
    """the blocks of M_ref_jtmj between different chains are exact zeros for both assets, with and without a mass-scale row, and the
    elimination the kernel uses equals the dense solve to 1e-10 of the largest |x|"""
    for c in cases.values():
        for e in range(N):
            M = c["M"][e]
            for a in FD.CHAINS:
                for b in FD.CHAINS:
                    if a is not b:
                        assert not M[a, b].any()
            x = FD.block_arrow_solve(M, c["force"][e])
            want = np.linalg.solve(M, c["force"][e])
            assert np.abs(x - want).max() <= 1e-10 * np.abs(want).max()
        assert np.linalg.cond(c["M"]).max() < 1e4


def test_the_reference_is_sensitive(cases):
    """a dropped armature and a dropped mass-scale row each move the result by more than the bar the GPU is held to (per block: 3x the
    worst error of the fp32 evaluation + 2 fp32 ulps of the largest |reference|), on the envs that carry a mass-scale row"""
    for asset, c in cases.items():
        for fixed in (False, True):
            base = _fd(c, FD.BIAS_ALL, fixed, M=c["M"])
            r32 = _fd(c, FD.BIAS_ALL, fixed, dtype=np.float32).astype(np.float64)
            moved = {"armature": _fd(c, FD.BIAS_ALL, fixed, armature=0.0), "mass scale": _fd(c, FD.BIAS_ALL, fixed, scale=None)}
            for name, sl in FD.BLOCKS:
                if fixed and sl.stop <= 6:
                    continue
                bar = 3.0 * np.abs(r32[:, sl] - base[:, sl]).max() + 2.0 * ulp32(np.abs(base[:, sl]).max())
                for what, m in moved.items():
                    shift = np.abs(m[N // 2:, sl] - base[N // 2:, sl]).max()
                    print("FD_SENSITIVE", asset, "fixed" if fixed else "floating", name, what, "shift / bar = %.3g" % (shift / bar))
                    assert shift > bar, (asset, fixed, name, what, shift, bar)
