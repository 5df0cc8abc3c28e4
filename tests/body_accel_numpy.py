"""References for bez_sim_body_accelerations (include/bez_sim.h "Body accelerations"): J_b udot + Jdot_b u - g of every rigid body of the
robot, rows [acceleration of the body's origin (classical, not spatial); angular acceleration], in the generalised velocity
u = [root_lin(3), root_ang(3), qd(18)].  Test-only.

  acc_ref        a forward recursion in LINK-LOCAL coordinates with Pluecker transforms, on the helpers of tests/inverse_dynamics_numpy.py
                 (the outward half of its rnea): spatial velocity v_i and acceleration a_i of every link in its own frame, base
                 acceleration a0 = [wdot; vdot - w x v]; a body at offset o of its link reads a_lin + alpha x o + w x (v_lin + w x o) in the
                 link's frame, which is the body's own.  A different formulation from the HIP kernel's.
  acc_ref_world  the same quantity written separately in WORLD axes about the root origin: joint axes and origins in world axes,
                 S = [a; r x a], A_i = A_p + S qdd + V_i x S qd, rows A.l + A.a x x + w x (V.l + w x x).
  A term is dropped by zeroing its input (udot; the velocities; g); the result is (udot + velocity) + gravity.  dtype=np.float64 is the
  reference; the fp32 yardstick of the GPU bars is the WORSE of the two formulations evaluated in np.float32 (yardstick_error): the frame
  a formula works in is a property of the problem's fp32 conditioning, not of the code under test.
  J_ref          the Jacobian of the bodies' origins from forward kinematics alone (fp64): what acc_ref is held to in
                 tests/test_body_accelerations_cpu.py -- J_ref @ udot, and central differences of J_ref @ u along a trajectory.
The quaternion is used as it is given (not renormalised), as the kernels use it."""
import numpy as np

from tests import dynamics_numpy as D
from tests.inverse_dynamics_numpy import _T, _crm, _mv, _plux, _quat_to_mat, _skew

ACC_UDOT, ACC_VELOCITY, ACC_GRAVITY, ACC_MOTION, ACC_ALL = 1, 2, 4, 3, 7
SPACE_ENV, SPACE_LOCAL = 0, 1
NG = 24
BLOCKS = (("linear", slice(0, 3)), ("angular", slice(3, 6)))


def model_of(asset):
    return D.model_of(asset)


def _joint_rotation(L, th, f):
    """(n,) joint angles -> (n, 3, 3): the child frame in the parent's"""
    K = _skew(np.asarray(L["axis"], f), f)
    th = th[:, None, None]
    return np.eye(3, dtype=f) + np.sin(th) * K + (f(1) - np.cos(th)) * (K @ K)


def _inputs(root, dof, udot, gravity, terms, f):
    assert terms and not terms & ~ACC_ALL
    root, dof = np.asarray(root, f), np.asarray(dof, f)
    n = root.shape[0]
    zero = np.zeros((n, NG), f)
    udot = zero if (udot is None or not terms & ACC_UDOT) else np.asarray(udot, f)
    u = np.concatenate([root[:, 7:13], dof[:, :, 1]], axis=1) if terms & ACC_VELOCITY else zero
    g = np.broadcast_to(np.asarray(gravity, f), (n, 3)) if terms & ACC_GRAVITY else np.zeros((n, 3), f)
    return root[:, 3:7], dof[:, :, 0], u, udot, g, zero


def _local_pass(model, quat, q, u, udot, f, mutate=None):
    """one outward pass in link-local coordinates -> (rows (n, nb, 6) [linear; angular] in each body's own frame, Rw (n, nb, 3, 3))"""
    links = model["links"]
    nl = len(links)
    R0 = _quat_to_mat(quat, f)
    E0 = _T(R0)
    lin, ang = u[:, 0:3], u[:, 3:6]
    v, a, Rw = [None] * nl, [None] * nl, [None] * nl
    v[0] = np.concatenate([_mv(E0, ang), _mv(E0, lin)], axis=1)
    a[0] = np.concatenate([_mv(E0, udot[:, 3:6]), _mv(E0, udot[:, 0:3] - np.cross(ang, lin))], axis=1)
    Rw[0] = R0
    eye = np.eye(3, dtype=f)
    for i in range(1, nl):
        L = links[i]
        p = L["parent"]
        Rj = _joint_rotation(L, q[:, i - 1], f)
        Xup = _plux(_T(Rj), np.zeros(3, f), f) @ _plux(eye, np.asarray(L["xyz"], f), f)
        S = np.concatenate([np.asarray(L["axis"], f), np.zeros(3, f)])
        vJ = S * u[:, 5 + i][:, None]
        v[i] = _mv(Xup, v[p]) + vJ
        cb = _mv(_crm(v[i], f), vJ)
        a[i] = _mv(Xup, a[p]) + S * udot[:, 5 + i][:, None] + (-cb if mutate == "cb_negated" else cb)
        Rw[i] = Rw[p] @ Rj
    nb = len(model["body_link"])
    rows = np.zeros((quat.shape[0], nb, 6), f)
    for b, (l, o) in enumerate(zip(model["body_link"], model["body_offset"])):
        o = np.zeros(3, f) if mutate == "offset_ignored" else np.asarray(o, f)
        w, vl, al, aL = v[l][:, 0:3], v[l][:, 3:6], a[l][:, 0:3], a[l][:, 3:6]
        rows[:, b, 0:3] = aL + np.cross(al, o)
        if mutate != "w_x_vp_dropped":
            rows[:, b, 0:3] += np.cross(w, vl + np.cross(w, o))
        rows[:, b, 3:6] = al
    return rows, np.stack([Rw[l] for l in model["body_link"]], axis=1)


def acc_ref(model, root, dof, udot, gravity, terms=ACC_MOTION, space=SPACE_ENV, dtype=np.float64, mutate=None):
    """root (n, 13) ROOT_STATE rows of the robot, dof (n, 18, 2), udot (n, 24) or None, gravity (3,) or (n, 3) -> (n, NB, 6) in `dtype`.
    mutate: one of the slips the sensitivity check plants ("w_x_vp_dropped", "cb_negated", "offset_ignored")."""
    f = dtype
    quat, q, u, udot, g, zero = _inputs(root, dof, udot, gravity, terms, f)
    ri, Rw = _local_pass(model, quat, q, zero, udot, f, mutate)
    rv, _ = _local_pass(model, quat, q, u, zero, f, mutate)
    motion = ri + rv
    out = np.zeros_like(motion)
    for sl in (slice(0, 3), slice(3, 6)):
        gl = -g[:, None, :] if sl.start == 0 else np.zeros((1, 1, 3), f)
        if space == SPACE_LOCAL:
            out[:, :, sl] = motion[:, :, sl] + _mv(_T(Rw), np.broadcast_to(gl, motion[:, :, sl].shape))
        else:
            out[:, :, sl] = _mv(Rw, motion[:, :, sl]) + gl
    assert out.dtype == f
    return out


def _world_pass(model, quat, q, u, udot, f):
    """one outward pass in world axes about the root origin -> (rows (n, nb, 6) in world axes, Rw (n, nb, 3, 3))"""
    links = model["links"]
    nl = len(links)
    n = quat.shape[0]
    E, r, w, v, al, aL = ([None] * nl for _ in range(6))
    E[0] = _quat_to_mat(quat, f)
    r[0] = np.zeros((n, 3), f)
    w[0], v[0] = u[:, 3:6], u[:, 0:3]
    al[0], aL[0] = udot[:, 3:6], udot[:, 0:3] - np.cross(u[:, 3:6], u[:, 0:3])
    for i in range(1, nl):
        L = links[i]
        p = L["parent"]
        axis = _mv(E[p], np.broadcast_to(np.asarray(L["axis"], f), (n, 3)))
        r[i] = r[p] + _mv(E[p], np.broadcast_to(np.asarray(L["xyz"], f), (n, 3)))
        E[i] = E[p] @ _joint_rotation(L, q[:, i - 1], f)
        Sa, Sl = axis, np.cross(r[i], axis)
        qd, qdd = u[:, 5 + i][:, None], udot[:, 5 + i][:, None]
        w[i], v[i] = w[p] + Sa * qd, v[p] + Sl * qd
        # V x (S qd) = [w x Sa ; w x Sl + v x Sa] qd
        al[i] = al[p] + Sa * qdd + np.cross(w[i], Sa) * qd
        aL[i] = aL[p] + Sl * qdd + (np.cross(w[i], Sl) + np.cross(v[i], Sa)) * qd
    nb = len(model["body_link"])
    rows = np.zeros((n, nb, 6), f)
    for b, (l, o) in enumerate(zip(model["body_link"], model["body_offset"])):
        x = r[l] + _mv(E[l], np.broadcast_to(np.asarray(o, f), (n, 3)))
        rows[:, b, 0:3] = aL[l] + np.cross(al[l], x) + np.cross(w[l], v[l] + np.cross(w[l], x))
        rows[:, b, 3:6] = al[l]
    return rows, np.stack([E[l] for l in model["body_link"]], axis=1)


def acc_ref_world(model, root, dof, udot, gravity, terms=ACC_MOTION, space=SPACE_ENV, dtype=np.float64):
    """acc_ref, written separately in world axes about the root origin"""
    f = dtype
    quat, q, u, udot, g, zero = _inputs(root, dof, udot, gravity, terms, f)
    ri, Rw = _world_pass(model, quat, q, zero, udot, f)
    rv, _ = _world_pass(model, quat, q, u, zero, f)
    out = ri + rv
    out[:, :, 0:3] = out[:, :, 0:3] - g[:, None, :]
    if space == SPACE_LOCAL:
        out = np.concatenate([_mv(_T(Rw), out[:, :, 0:3]), _mv(_T(Rw), out[:, :, 3:6])], axis=2)
    assert out.dtype == f
    return out


def yardstick_error(model, root, dof, udot, gravity, terms, space, ref64):
    """(2,) per block (rows 0:3, rows 3:6): the worst absolute error against ref64 of the WORSE of the two formulations in np.float32"""
    worst = np.zeros(2)
    for fn in (acc_ref, acc_ref_world):
        r32 = fn(model, root, dof, udot, gravity, terms, space, np.float32).astype(np.float64)
        for k, (_, sl) in enumerate(BLOCKS):
            worst[k] = max(worst[k], float(np.abs(r32[:, :, sl] - ref64[:, :, sl]).max()))
    return worst


def body_rotations(model, quat, q):
    """(nb, 3, 3) fp64: the orientation of every body of one state"""
    return _world_pass(model, np.asarray(quat, np.float64)[None], np.asarray(q, np.float64)[None], np.zeros((1, NG)), np.zeros((1, NG)), np.float64)[1][0]


def J_ref(model, R0, q):
    """(nb, 6, 24) fp64 from forward kinematics alone, for one state with the root's rotation MATRIX R0 (3, 3) and joint angles q (18,):
    rows 0:3 the velocity of the body's origin, rows 3:6 its angular velocity, columns u = [root_lin, root_ang, qd]"""
    links = model["links"]
    nl = len(links)
    E, r, a = [None] * nl, [None] * nl, [None] * nl
    E[0], r[0] = np.asarray(R0, np.float64), np.zeros(3)
    skew = lambda v: np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]], np.float64)
    for i in range(1, nl):
        L = links[i]
        p = L["parent"]
        K = skew(np.asarray(L["axis"], np.float64))
        r[i] = r[p] + E[p] @ np.asarray(L["xyz"], np.float64)
        a[i] = E[p] @ np.asarray(L["axis"], np.float64)
        E[i] = E[p] @ (np.eye(3) + np.sin(q[i - 1]) * K + (1.0 - np.cos(q[i - 1])) * (K @ K))
    nb = len(model["body_link"])
    J = np.zeros((nb, 6, NG))
    for b, (l, o) in enumerate(zip(model["body_link"], model["body_offset"])):
        x = r[l] + E[l] @ np.asarray(o, np.float64)
        J[b, 0:3, 0:3] = np.eye(3)
        J[b, 3:6, 3:6] = np.eye(3)
        J[b, 0:3, 3:6] = -skew(x)
        j = l
        while j > 0:
            J[b, 0:3, 5 + j] = np.cross(a[j], x - r[j])
            J[b, 3:6, 5 + j] = a[j]
            j = links[j]["parent"]
    return J
