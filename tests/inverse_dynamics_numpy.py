"""References for bez_sim_inverse_dynamics (include/bez_sim.h "Inverse dynamics"): M(q) udot + h(q, u) in the generalised velocity
u = [root_lin(3), root_ang(3), qd(18)], world axes, rows [force; moment about the root origin; joint torques].  Test-only.

  rnea        Featherstone's recursive Newton-Euler algorithm for a floating base in LINK-LOCAL coordinates with Pluecker transforms, the
              route of tests/rbd_numpy.rnea_floating written out in the dtype it is given (tests/test_inverse_dynamics_cpu.py holds the
              fp64 evaluation to rbd_numpy's).  A different formulation from the HIP kernel's (world axes about the root origin).
  id_ref      the call's result from it: a term is dropped by zeroing its input (udot; the velocities; g), the base acceleration is
              a0 = [wdot; vdot - w x v] as tests/dof_force_numpy.rnea_torques forms it, the base wrench f0 is rotated to world axes and
              reordered, the armature joins the joint rows.  dtype=np.float64 is the reference, dtype=np.float32 the yardstick of fp32
              rounding for the GPU bars.
The quaternion is used as it is given (not renormalised), as tests/dynamics_numpy.M_ref_jtmj and the kernels use it."""
import numpy as np

from tests import dynamics_numpy as D

ID_INERTIA, ID_VELOCITY, ID_GRAVITY, ID_ALL = 1, 2, 4, 7
NG = 24
BLOCKS = (("force", slice(0, 3)), ("moment", slice(3, 6)), ("joints", slice(6, NG)))


def _skew(v, f):
    """(..., 3) -> (..., 3, 3)"""
    v = np.asarray(v, f)
    K = np.zeros(v.shape[:-1] + (3, 3), f)
    K[..., 0, 1], K[..., 0, 2], K[..., 1, 0] = -v[..., 2], v[..., 1], v[..., 2]
    K[..., 1, 2], K[..., 2, 0], K[..., 2, 1] = -v[..., 0], -v[..., 1], v[..., 0]
    return K


def _mv(A, x):
    return (A @ x[..., None])[..., 0]


def _T(A):
    return np.swapaxes(A, -1, -2)


def _quat_to_mat(q, f):
    q = np.asarray(q, f)
    x, y, z, w = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    one, two = f(1), f(2)
    R = np.zeros(q.shape[:-1] + (3, 3), f)
    R[..., 0, 0] = one - two * (y * y + z * z); R[..., 0, 1] = two * (x * y - z * w); R[..., 0, 2] = two * (x * z + y * w)
    R[..., 1, 0] = two * (x * y + z * w); R[..., 1, 1] = one - two * (x * x + z * z); R[..., 1, 2] = two * (y * z - x * w)
    R[..., 2, 0] = two * (x * z - y * w); R[..., 2, 1] = two * (y * z + x * w); R[..., 2, 2] = one - two * (x * x + y * y)
    return R


def _plux(E, r, f):
    E = np.asarray(E, f)
    X = np.zeros(E.shape[:-2] + (6, 6), f)
    X[..., :3, :3] = E
    X[..., 3:, 3:] = E
    X[..., 3:, :3] = -(E @ _skew(r, f))
    return X


def _crm(v, f):
    X = np.zeros(v.shape[:-1] + (6, 6), f)
    X[..., :3, :3] = _skew(v[..., :3], f)
    X[..., 3:, 3:] = _skew(v[..., :3], f)
    X[..., 3:, :3] = _skew(v[..., 3:], f)
    return X


def _link_inertia(L, scale, f):
    """scale (n,) -> (n, 6, 6)"""
    m = (f(L["mass"]) * scale)[:, None, None]
    c = np.asarray(L["com"], f)
    xx, yy, zz, xy, xz, yz = [f(v) for v in L["inertia"]]
    Ic = np.array([[xx, xy, xz], [xy, yy, yz], [xz, yz, zz]], f) * scale[:, None, None]
    Cx = _skew(c, f)
    I = np.zeros((scale.shape[0], 6, 6), f)
    I[:, :3, :3] = Ic + m * (Cx @ Cx.T)
    I[:, :3, 3:] = m * Cx
    I[:, 3:, :3] = m * Cx.T
    I[:, 3:, 3:] = m * np.eye(3, dtype=f)
    return I


def rnea(links, quat, v0, a0, q, qd, qdd, gravity, scale=None, dtype=np.float64):
    """tests/rbd_numpy.rnea_floating in `dtype`, over a batch of n states: quat (n, 4); v0 (n, 6) = [w; v] of the torso origin and a0
    (n, 6) its spatial acceleration, world axes; q, qd, qdd (n, 18); gravity (n, 3); `scale` (n, 19) mass-scale rows (masses and inertias
    alike) or None.  Returns (f0 (n, 6) [moment; force] in BASE coordinates, tau (n, 18))."""
    f = dtype
    nl = len(links)
    quat, v0, a0, q, qd, qdd, gravity = (np.asarray(x, f) for x in (quat, v0, a0, q, qd, qdd, gravity))
    n = quat.shape[0]
    scale = np.ones((n, nl), f) if scale is None else np.asarray(scale, f)
    E0 = _T(_quat_to_mat(quat, f))
    R0 = np.zeros((n, 6, 6), f)
    R0[:, :3, :3] = E0
    R0[:, 3:, 3:] = E0
    v, a, F, Xup, S = [None] * nl, [None] * nl, [None] * nl, [None] * nl, [None] * nl
    I = [_link_inertia(L, scale[:, i], f) for i, L in enumerate(links)]
    bias = lambda i: _mv(-_T(_crm(v[i], f)), _mv(I[i], v[i]))   # v x* I v
    v[0] = _mv(R0, v0)
    ag = np.concatenate([np.zeros((n, 3), f), gravity], axis=1)
    a[0] = _mv(R0, a0 - ag)
    F[0] = _mv(I[0], a[0]) + bias(0)
    eye = np.eye(3, dtype=f)
    for i in range(1, nl):
        L = links[i]
        p = L["parent"]
        axis = np.asarray(L["axis"], f)
        K = _skew(axis, f)
        th = q[:, i - 1][:, None, None]
        Rj = eye + np.sin(th) * K + (f(1) - np.cos(th)) * (K @ K)
        Xup[i] = _plux(_T(Rj), np.zeros(3, f), f) @ _plux(eye, np.asarray(L["xyz"], f), f)
        S[i] = np.concatenate([axis, np.zeros(3, f)])
        vJ = S[i] * qd[:, i - 1][:, None]
        v[i] = _mv(Xup[i], v[p]) + vJ
        a[i] = _mv(Xup[i], a[p]) + S[i] * qdd[:, i - 1][:, None] + _mv(_crm(v[i], f), vJ)
        F[i] = _mv(I[i], a[i]) + bias(i)
    tau = np.zeros((n, nl - 1), f)
    for i in range(nl - 1, 0, -1):
        tau[:, i - 1] = F[i] @ S[i]
        p = links[i]["parent"]
        F[p] = F[p] + _mv(_T(Xup[i]), F[i])
    assert F[0].dtype == f and tau.dtype == f
    return F[0], tau


def id_ref_batch(model, root, dof, udot, gravity, mass_scale, armature, terms, dtype=np.float64):
    """id_ref over n envs: root (n, 13) ROOT_STATE rows of the robot, dof (n, 18, 2), udot (n, 24) or None, gravity (3,) or (n, 3),
    mass_scale (n, 19) or None -> (n, 24) in `dtype`"""
    f = dtype
    assert terms and not terms & ~ID_ALL
    root, dof = np.asarray(root, f), np.asarray(dof, f)
    n = root.shape[0]
    udot = np.zeros((n, NG), f) if (udot is None or not terms & ID_INERTIA) else np.asarray(udot, f)
    v0 = root[:, 7:13] if terms & ID_VELOCITY else np.zeros((n, 6), f)
    qd = dof[:, :, 1] if terms & ID_VELOCITY else np.zeros((n, 18), f)
    g = np.broadcast_to(np.asarray(gravity, f), (n, 3)) if terms & ID_GRAVITY else np.zeros((n, 3), f)
    lin, ang = v0[:, 0:3], v0[:, 3:6]
    a0 = np.concatenate([udot[:, 3:6], udot[:, 0:3] - np.cross(ang, lin)], axis=1)
    f0, tau = rnea(model["links"], root[:, 3:7], np.concatenate([ang, lin], axis=1), a0, dof[:, :, 0], qd, udot[:, 6:], g, mass_scale, f)
    Rw = _quat_to_mat(root[:, 3:7], f)
    out = np.concatenate([_mv(Rw, f0[:, 3:6]), _mv(Rw, f0[:, 0:3]), tau + f(armature) * udot[:, 6:]], axis=1)
    assert out.dtype == f
    return out


def id_ref(model, quat, v0, q, qd, udot, gravity, mass_scale=None, armature=0.0, terms=ID_ALL, dtype=np.float64):
    """(24,) in `dtype` for one state.  v0 = u[0:6] = [root_lin, root_ang] (ROOT_STATE columns 7:13), udot (24,) or None for zero,
    gravity (3,), mass_scale (19,) or None, `terms` a set of ID_* bits."""
    root = np.zeros((1, 13), dtype)
    root[0, 3:7], root[0, 7:13] = quat, v0
    dof = np.stack([np.asarray(q, dtype), np.asarray(qd, dtype)], axis=-1)[None]
    return id_ref_batch(model, root, dof, None if udot is None else np.asarray(udot, dtype)[None], gravity,
                        None if mass_scale is None else np.asarray(mass_scale, dtype)[None], armature, terms, dtype)[0]
