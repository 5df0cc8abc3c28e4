"""CPU: the references that pin the rigid-body refresh (tests/test_gpu_state_tensors.py) on the state set they are evaluated on
(both in tests/state_sets.py: generate_states, fd_reference, oracle_rows).

What is asserted here: the state set reaches every branch of mat_to_quat (10 % of the body rotations at least, each), the fp64
oracle agrees with the FD reference to fp32 output rounding (which settles which point's velocity the body rows carry: the body
origin's), and a numpy copy of mat_to_quat with one sign or index slipped in any branch fails the comparison on these states."""
import numpy as np
import pytest

from bez_isaacgym_amd import abi
from tests.state_sets import (DOF_LOWER, DOF_UPPER, FIELDS, NB, align_quat, fd_reference, field_errors, generate_states,
                              oracle_rows, quat_mat, ulp32)   # noqa: F401  (oracle_rows: tests/test_dynamics_cpu.py takes it from here)

# ---------------------------------------------------------------- mat_to_quat, written out in numpy (fp32 arithmetic like the kernel)

def mat_to_quat_branch(R):
    """which branch of bez_sim.hip mat_to_quat a rotation takes: 0 trace > 0, 1 m00, 2 m11, 3 m22"""
    R = np.asarray(R, np.float32)
    m00, m11, m22 = R[..., 0, 0], R[..., 1, 1], R[..., 2, 2]
    tr = m00 + m11 + m22
    return np.where(tr > 0, 0, np.where((m00 > m11) & (m00 > m22), 1, np.where(m11 > m22, 2, 3)))


def mat_to_quat_np(R, mutant=None):
    """mat_to_quat of bez_sim.hip / oracle/bez_oracle.c.  mutant = (branch, kind): one sign ("sign") or one index ("index") slipped
    in that branch -- the sensitivity check of the state set."""
    R = np.asarray(R, np.float32)
    f = np.float32
    m = lambda i, j: R[..., i, j]
    br = mat_to_quat_branch(R)
    out = np.zeros(R.shape[:-2] + (4,), np.float32)
    mut = lambda b, k: mutant == (b, k)
    with np.errstate(divide="ignore", invalid="ignore"):
        # trace > 0
        s = np.sqrt(m(0, 0) + m(1, 1) + m(2, 2) + f(1)) * f(2)
        q0 = np.stack([(m(2, 1) - m(1, 2)) / s, (m(0, 2) - m(2, 0)) / s,
                       ((m(1, 0) + m(0, 1)) if mut(0, "sign") else (m(1, 0) - m(0, 1))) / s, f(0.25) * s], -1)
        if mut(0, "index"):
            q0[..., 1] = (m(0, 2) - m(0, 1)) / s
        # m00 largest
        s = np.sqrt(f(1) + m(0, 0) - m(1, 1) - m(2, 2)) * f(2)
        q1 = np.stack([f(0.25) * s, (m(0, 1) + m(1, 0)) / s, ((m(0, 2) - m(2, 0)) if mut(1, "sign") else (m(0, 2) + m(2, 0))) / s,
                       (m(2, 1) - m(1, 2)) / s], -1)
        if mut(1, "index"):
            q1[..., 3] = (m(2, 1) - m(0, 2)) / s
        # m11 largest
        s = np.sqrt(f(1) + m(1, 1) - m(0, 0) - m(2, 2)) * f(2)
        q2 = np.stack([(m(0, 1) + m(1, 0)) / s, f(0.25) * s, (m(1, 2) + m(2, 1)) / s,
                       ((m(0, 2) + m(2, 0)) if mut(2, "sign") else (m(0, 2) - m(2, 0))) / s], -1)
        if mut(2, "index"):
            q2[..., 2] = (m(1, 2) + m(1, 0)) / s
        # m22 largest
        s = np.sqrt(f(1) + m(2, 2) - m(0, 0) - m(1, 1)) * f(2)
        q3 = np.stack([(m(0, 2) + m(2, 0)) / s, ((m(1, 2) - m(2, 1)) if mut(3, "sign") else (m(1, 2) + m(2, 1))) / s, f(0.25) * s,
                       (m(1, 0) - m(0, 1)) / s], -1)
        if mut(3, "index"):
            q3[..., 0] = (m(0, 2) + m(2, 1)) / s
    for b, qb in enumerate((q0, q1, q2, q3)):
        out[br == b] = qb[br == b]
    return out


# ---------------------------------------------------------------- tests

@pytest.fixture(scope="module")
def states():
    return generate_states(300)


@pytest.fixture(scope="module")
def reference(states):
    return fd_reference(states[0], states[1])


def test_fixture_limits_are_the_models(states):
    """the generator's joint range is the URDF's, which is the range the model tables bake (BEZ_DOF_LOWER / BEZ_DOF_UPPER)"""
    import json
    import os
    model = json.load(open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bez_isaacgym_amd", "model",
                                        "bez_model.json")))
    np.testing.assert_array_equal(np.float32(model["dof_lower"]), np.float32(DOF_LOWER))
    np.testing.assert_array_equal(np.float32(model["dof_upper"]), np.float32(DOF_UPPER))
    root, dof, cases = states
    assert root.dtype == dof.dtype == np.float32 and len(cases) == root.shape[0] == dof.shape[0]
    q = dof[:, :, 0]
    assert (q >= np.float32(DOF_LOWER)).all() and (q <= np.float32(DOF_UPPER)).all()
    assert (q == np.float32(DOF_LOWER)).any(axis=0).all() and (q == np.float32(DOF_UPPER)).any(axis=0).all()
    assert np.abs(root[:, 0:2]).max() > 90 and np.abs(dof[:, :, 1]).max() > 19 and np.abs(root[:, 10:13]).max() > 9
    assert (root[:, 6] == 0).sum() >= 10 and (root[:, 6] < 0).sum() >= 0.3 * len(cases)


def test_states_reach_every_mat_to_quat_branch(states, reference):
    """of all 300 x 21 body rotations, every branch of mat_to_quat takes 10 % at least"""
    root, dof, _ = states
    Rb = np.array([[quat_mat(q) for q in env] for env in reference[:, :, 3:7]])
    share = np.bincount(mat_to_quat_branch(Rb).ravel(), minlength=4) / Rb[..., 0, 0].size
    assert (share >= 0.10).all(), share
    seam = np.array([quat_mat(q) for q in root[:32, 3:7].astype(np.float64)])
    assert set(mat_to_quat_branch(seam)) == {0, 1, 2, 3}


def test_fp64_oracle_matches_fd_reference(states):
    """default asset: on the state set with its quaternions made exactly unit in fp64, the fp64 oracle's rows agree with the FD
    reference to their fp32 output rounding (half an ulp, elementwise): the body rows carry the velocity of the body ORIGIN, and
    the reference is accurate far below fp32 rounding.  (With the fp32 inputs as they are, |q| - 1 ~ 6e-8 moves both by ~1e-7
    relative, differently: the GPU bars take that from the fp32 oracle's error on the same states.)"""
    from oracle.bez_oracle import Oracle
    root, dof = states[0].astype(np.float64), states[1].astype(np.float64)
    root[:, 3:7] /= np.linalg.norm(root[:, 3:7], axis=1, keepdims=True)
    n = root.shape[0]
    ref = fd_reference(root, dof)
    o = Oracle(abi.default_config(n))
    for e in range(n):
        r = root[e]
        o.set_env_state_f64(e, r[0:3], r[3:7], r[7:10], r[10:13], dof[e, :, 0], dof[e, :, 1])
    o64 = o.rigid_body_states.reshape(n, o.nbe, 13)[:, :NB]
    err = field_errors(o64, ref)
    for name, sl in FIELDS:
        bar = 0.51 * ulp32(ref[..., sl]) + 1e-10
        bad = err[name] > bar
        assert not bad.any(), (name, float(err[name].max()), np.argwhere(bad)[:5])


def test_numpy_mat_to_quat_matches_reference(states, reference):
    """the numpy copy of the kernel's mat_to_quat, in fp32, on the reference's rotations: within 4 fp32 ulps of 1"""
    Rb = np.array([[quat_mat(q) for q in env] for env in reference[:, :, 3:7]])
    qk = mat_to_quat_np(Rb)
    err = np.abs(align_quat(qk, reference[..., 3:7]) - reference[..., 3:7])
    assert err.max() <= 4 * 2.0 ** -24 * 2, float(err.max())


@pytest.mark.parametrize("branch", [0, 1, 2, 3])
@pytest.mark.parametrize("kind", ["sign", "index"])
def test_state_set_catches_a_slip_in_every_branch(states, reference, branch, kind):
    """one sign or one index slipped in any one branch of mat_to_quat fails the quaternion bar on these states"""
    Rb = np.array([[quat_mat(q) for q in env] for env in reference[:, :, 3:7]])
    qk = mat_to_quat_np(Rb, mutant=(branch, kind))
    err = np.nan_to_num(np.abs(align_quat(qk, reference[..., 3:7]) - reference[..., 3:7]), nan=1.0)
    assert err.max() > 1e-3, (branch, kind, float(err.max()))
