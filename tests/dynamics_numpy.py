"""fp64 references for the dynamics tensors (include/bez_sim.h "Dynamics tensors"): the Jacobian of the robot's bodies and the mass
matrix, both in the generalised velocity u = [root_lin(3), root_ang(3), qd(18)], world axes.  Test-only.

  J_ref_oracle / J_ref_fd   column k of J is what the body rows carry as origin velocity (rows 0:3) and angular velocity (rows 3:6) in
                            the state whose generalised velocity is the unit vector e_k: from the CPU oracle's rigid-body rows (every
                            asset, fp64 or fp32 build) and from the finite-difference FK of tests/state_sets.fd_reference
                            (default asset; the URDF fixture, not the model tables).
  M_ref_rnea                column k of M is the generalised force of tests/rbd_numpy.rnea_floating at zero velocity and zero gravity
                            for the unit acceleration e_k; the base wrench is rotated to world axes and reordered to [force; moment
                            about the root origin].
  M_ref_jtmj                sum over links of J_com^T diag(m I3, I_c in world axes) J_com from the model JSON (its "cleats" entry for the
                            cleats asset), written out in the dtype it is given: fp64 is a reference, np.float32 is the yardstick of
                            fp32 rounding for the GPU bars.
  M_ref_kane                the same columns from tests/urdf_independent.generalized_force (default asset, 21 separate bodies).
All three take a (19,) mass-scale row (link masses and inertias alike) and the armature (added to the 18 joint diagonals)."""
import copy
import json
import os

import numpy as np

from tests import rbd_numpy as R
from tests import urdf_independent as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODEL = json.load(open(os.path.join(ROOT, "bez_isaacgym_amd", "model", "bez_model.json")))
NG = 24


def model_of(asset):
    """the link model of an asset: "default" and "box" share the stl asset's dynamics, "cleats" has heavier feet"""
    return MODEL["cleats"] if asset == "cleats" else MODEL


def unit_velocity_states(root, dof):
    """(n, 13), (n, 18, 2) -> (n * 24, 13), (n * 24, 18, 2): state e repeated 24 times, copy k with the generalised velocity e_k"""
    n = root.shape[0]
    r = np.repeat(np.asarray(root), NG, axis=0).copy()
    d = np.repeat(np.asarray(dof), NG, axis=0).copy()
    r[:, 7:13] = 0
    d[:, :, 1] = 0
    k = np.tile(np.arange(NG), n)
    rows = np.arange(n * NG)
    base = k < 6
    r[rows[base], 7 + k[base]] = 1
    d[rows[~base], k[~base] - 6, 1] = 1
    return r, d


def _columns(rows, n, nb):
    """body rows (n * 24, >= nb, 13) of the unit-velocity states -> J (n, nb, 6, 24)"""
    v = rows[:, :nb, 7:13].reshape(n, NG, nb, 6)
    return np.ascontiguousarray(np.transpose(v, (0, 2, 3, 1))).astype(np.float64)


def J_ref_oracle(make_cfg, precision, root, dof, nb):
    """make_cfg(num_envs) -> the oracle's config for the asset and task; nb robot bodies (the ball's row, if any, is dropped)"""
    from tests.state_sets import oracle_rows
    r, d = unit_velocity_states(root, dof)
    return _columns(oracle_rows(make_cfg(r.shape[0]), precision, r, d), root.shape[0], nb)


def J_ref_fd(root, dof):
    from tests.state_sets import NB, fd_reference
    r, d = unit_velocity_states(root, dof)
    return _columns(fd_reference(r, d), root.shape[0], NB)


# ---------------------------------------------------------------- M, three ways

def scaled_model(model, mass_scale):
    m = {"links": copy.deepcopy(model["links"])}
    for L, s in zip(m["links"], np.asarray(mass_scale, np.float64)):
        L["mass"] = L["mass"] * s
        L["inertia"] = [x * s for x in L["inertia"]]
    return m


def _with_armature(M, armature):
    M = M.copy()
    M[np.arange(6, NG), np.arange(6, NG)] += armature
    return M


def M_ref_rnea(model, quat, q, mass_scale=None, armature=0.0):
    mdl = model if mass_scale is None else scaled_model(model, mass_scale)
    quat = np.asarray(quat, np.float64)
    q = np.asarray(q, np.float64)
    Rw = R.quat_to_mat(quat)
    M = np.zeros((NG, NG))
    z18, z3 = np.zeros(18), np.zeros(3)
    for k in range(NG):
        a0, qdd = np.zeros(6), np.zeros(18)
        if k < 3:
            a0[3 + k] = 1      # [angular; linear] of the torso origin, world axes
        elif k < 6:
            a0[k - 3] = 1
        else:
            qdd[k - 6] = 1
        f0, tau = R.rnea_floating(mdl, quat, np.zeros(6), a0, q, z18, qdd, z3)
        M[0:3, k] = Rw @ f0[3:6]
        M[3:6, k] = Rw @ f0[0:3]
        M[6:, k] = tau
    return _with_armature(M, armature)


def M_ref_jtmj(model, quat, q, mass_scale=None, armature=0.0, dtype=np.float64, mutate=None):
    """every operation in `dtype`.  mutate: a function applied to the list of link dicts first (the sensitivity checks)"""
    f = dtype
    links = copy.deepcopy(model["links"])
    if mutate is not None:
        mutate(links)
    n = len(links)
    scale = np.ones(n, f) if mass_scale is None else np.asarray(mass_scale, f)
    x, y, z, w = [f(v) for v in np.asarray(quat, f)]
    one, two = f(1), f(2)
    E = [None] * n
    r = [None] * n
    a = [None] * n
    E[0] = np.array([[one - two * (y * y + z * z), two * (x * y - z * w), two * (x * z + y * w)],
                     [two * (x * y + z * w), one - two * (x * x + z * z), two * (y * z - x * w)],
                     [two * (x * z - y * w), two * (y * z + x * w), one - two * (x * x + y * y)]], f)
    r[0] = np.zeros(3, f)
    skew = lambda v: np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]], f)
    M = np.zeros((NG, NG), f)
    for i, L in enumerate(links):
        if i > 0:
            p = L["parent"]
            ax = np.asarray(L["axis"], f)
            K = skew(ax)
            th = f(q[i - 1])
            r[i] = r[p] + E[p] @ np.asarray(L["xyz"], f)
            a[i] = E[p] @ ax
            E[i] = E[p] @ (np.eye(3, dtype=f) + np.sin(th) * K + (one - np.cos(th)) * (K @ K))
        c = r[i] + E[i] @ np.asarray(L["com"], f)
        Jc = np.zeros((6, NG), f)
        Jc[0:3, 0:3] = np.eye(3, dtype=f)
        Jc[3:6, 3:6] = np.eye(3, dtype=f)
        Jc[0:3, 3:6] = -skew(c)
        j = i
        while j > 0:
            Jc[0:3, 5 + j] = np.cross(a[j], c - r[j])
            Jc[3:6, 5 + j] = a[j]
            j = links[j]["parent"]
        xx, yy, zz, xy, xz, yz = [f(v) for v in L["inertia"]]
        Ic = E[i] @ (np.array([[xx, xy, xz], [xy, yy, yz], [xz, yz, zz]], f) * scale[i]) @ E[i].T
        W = np.zeros((6, 6), f)
        W[0:3, 0:3] = np.eye(3, dtype=f) * (f(L["mass"]) * scale[i])
        W[3:6, 3:6] = Ic
        M = M + Jc.T @ W @ Jc
    M[np.arange(6, NG), np.arange(6, NG)] += f(armature)
    assert M.dtype == f
    return M


def scaled_bodies(bodies, mass_scale, body_link):
    out = copy.deepcopy(bodies)
    for B, l in zip(out, body_link):
        s = float(mass_scale[l])
        B["mass"] = B["mass"] * s
        B["inertia"] = (np.asarray(B["inertia"], np.float64) * s).tolist()
    return out


def M_ref_kane(quat, q, mass_scale=None, armature=0.0):
    bodies = U.load_fixture()
    if mass_scale is not None:
        bodies = scaled_bodies(bodies, mass_scale, MODEL["body_link"])
    quat = np.asarray(quat, np.float64)
    q = np.asarray(q, np.float64)
    M = np.zeros((NG, NG))
    z3, z18 = np.zeros(3), np.zeros(18)
    for k in range(NG):
        dw, dv, qdd = np.zeros(3), np.zeros(3), np.zeros(18)
        if k < 3:
            dv[k] = 1
        elif k < 6:
            dw[k - 3] = 1
        else:
            qdd[k - 6] = 1
        g = U.generalized_force(bodies, z3, quat, z3, z3, q, z18, dw, dv, qdd, z3)
        M[0:3, k], M[3:6, k], M[6:, k] = g[3:6], g[0:3], g[6:]
    return _with_armature(M, armature)


def scale_of(M):
    """sqrt(M_ii M_jj): the size every |M_ij| of a positive definite M stays below (elementwise, over the last two axes)"""
    d = np.sqrt(np.abs(np.diagonal(np.asarray(M, np.float64), axis1=-2, axis2=-1)))
    return d[..., :, None] * d[..., None, :]
