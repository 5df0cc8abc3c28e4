"""The reference for bez_sim_forward_dynamics (include/bez_sim.h "Forward dynamics"): udot = M^-1 (f - h), put together from what the
project already trusts -- M from tests/dynamics_numpy.M_ref_jtmj, h from tests/inverse_dynamics_numpy.id_ref_batch with udot = 0 -- and a
dense np.linalg.solve, every operation in `dtype`.  It knows nothing of the tree: the kernel's block-arrow elimination is held to it.
Not a test."""
import numpy as np

from tests import dynamics_numpy as D
from tests import inverse_dynamics_numpy as ID

NG = ID.NG
BLOCKS = ID.BLOCKS
ID_INERTIA, ID_VELOCITY, ID_GRAVITY = 1, 2, 4
BIAS_ALL = ID_VELOCITY | ID_GRAVITY
# the DOF columns of the five chains off the torso: head, left arm, left leg, right arm, right leg
CHAINS = (slice(6, 8), slice(8, 10), slice(10, 16), slice(16, 18), slice(18, 24))


def M_batch(model, root, dof, scale, armature, dtype=np.float64, mutate=None):
    """(n, 24, 24) in `dtype`: M_ref_jtmj of every env; scale (n, 19) or None"""
    root, dof = np.asarray(root, dtype), np.asarray(dof, dtype)
    return np.stack([D.M_ref_jtmj(model, root[e, 3:7], dof[e, :, 0], None if scale is None else scale[e], armature, dtype, mutate)
                     for e in range(root.shape[0])])


def h_batch(model, root, dof, g, scale, armature, bias, dtype=np.float64):
    """(n, 24) in `dtype`: the terms of h(q, u) selected by `bias`; zeros for bias == 0"""
    if not bias:
        return np.zeros((np.asarray(root).shape[0], NG), dtype)
    return ID.id_ref_batch(model, root, dof, None, g, scale, armature, bias, dtype)


def fd_ref_batch(model, root, dof, force, g, scale, armature, bias, fixed_base, dtype=np.float64, M=None):
    """udot (n, 24) in `dtype`.  root (n, 13) ROOT_STATE rows of the robot, dof (n, 18, 2), force (n, 24) or None for zero, g (3,) or
    (n, 3), scale (n, 19) or None, bias a subset of ID_VELOCITY | ID_GRAVITY, fixed_base: rows 0:6 are zero and rows 6:24 solve
    M[6:, 6:] qdd = (f - h)[6:].  M: M_batch of the same arguments where the caller has it already."""
    f = dtype
    assert not bias & ~BIAS_ALL
    n = np.asarray(root).shape[0]
    if M is None:
        M = M_batch(model, root, dof, scale, armature, f)
    assert M.dtype == f
    rhs = (np.zeros((n, NG), f) if force is None else np.asarray(force, f)) - h_batch(model, root, dof, g, scale, armature, bias, f)
    out = np.zeros((n, NG), f)
    lo = 6 if fixed_base else 0
    out[:, lo:] = np.linalg.solve(M[:, lo:, lo:], rhs[:, lo:, None])[:, :, 0]
    assert out.dtype == f
    return out


def block_arrow_solve(M, rhs):
    """M^-1 rhs for one env by the elimination the kernel uses: per chain y_c = M_cc^-1 r_c and Z_c = M_cc^-1 B_c, the Schur complement
    S = M00 - sum_c B_c^T Z_c on the base, x_0 = S^-1 (r_0 - sum_c B_c^T y_c), x_c = y_c - Z_c x_0.  Right only where the blocks of M
    between different chains vanish."""
    S, g = M[0:6, 0:6].copy(), rhs[0:6].copy()
    y, Z = {}, {}
    for c in CHAINS:
        B = M[c, 0:6]
        y[c.start], Z[c.start] = np.linalg.solve(M[c, c], rhs[c]), np.linalg.solve(M[c, c], B)
        S -= B.T @ Z[c.start]
        g -= B.T @ y[c.start]
    x = np.zeros_like(rhs)
    x[0:6] = np.linalg.solve(S, g)
    for c in CHAINS:
        x[c] = y[c.start] - Z[c.start] @ x[0:6]
    return x
