"""Reference for bez_sim_centroidal (include/bez_sim.h "Centroidal dynamics"): centre of mass, momentum about it, the centroidal
momentum matrix A_G and the mechanical energy, in u = [root_lin(3), root_ang(3), qd(18)], world axes.  Test-only.

  cm_ref   built link by link from first principles, every operation in the dtype it is given: forward kinematics to each link's own
           centre of mass c_l and its velocity v_l (the velocity of the link's origin carried down the tree, then w_l x (c_l - r_l)), the
           link's angular velocity w_l and its inertia about c_l in world axes; then
             MASS = sum m_l,  c = sum m_l c_l / MASS,  LIN_MOM = sum m_l v_l,  ANG_MOM = sum (I_l w_l + m_l (c_l - c) x v_l),
             KINETIC = sum 1/2 (m_l |v_l|^2 + w_l . I_l w_l) + 1/2 armature |qd|^2,  POTENTIAL = -MASS g . COM,
           and A_G column by column: column k is [LIN_MOM; ANG_MOM] of the same configuration with the unit velocity u = e_k.
           Positions are relative to the root origin until COM = root_pos + c.  Nothing here reads a mass matrix:
           tests/dynamics_numpy.M_ref_jtmj is the cross-check of tests/test_centroidal_cpu.py, not the source.
           dtype=np.float64 is the reference, dtype=np.float32 the yardstick of fp32 rounding for the GPU bars.
The quaternion is used as it is given (not renormalised), as tests/dynamics_numpy.M_ref_jtmj and the kernels use it."""
import copy

import numpy as np

from tests import dynamics_numpy as D
from tests.inverse_dynamics_numpy import _mv
from tests.state_sets import generate_states

NG = 24
CM_WORDS = 16
CM_COM, CM_COM_VEL, CM_LIN_MOM, CM_ANG_MOM, CM_MASS, CM_KINETIC, CM_POTENTIAL = 0, 3, 6, 9, 12, 13, 14
STATE_BLOCKS = (("com", slice(0, 3)), ("com_vel", slice(3, 6)), ("lin_mom", slice(6, 9)), ("ang_mom", slice(9, 12)), ("mass", slice(12, 13)),
                ("kinetic", slice(13, 14)), ("potential", slice(14, 15)))
MATRIX_BLOCKS = (("matrix_lin", slice(0, 3)), ("matrix_ang", slice(3, 6)))


def _quat_to_mat(q, f):
    x, y, z, w = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    one, two = f(1), f(2)
    R = np.zeros((q.shape[0], 3, 3), f)
    R[:, 0, 0] = one - two * (y * y + z * z); R[:, 0, 1] = two * (x * y - z * w); R[:, 0, 2] = two * (x * z + y * w)
    R[:, 1, 0] = two * (x * y + z * w); R[:, 1, 1] = one - two * (x * x + z * z); R[:, 1, 2] = two * (y * z - x * w)
    R[:, 2, 0] = two * (x * z - y * w); R[:, 2, 1] = two * (y * z + x * w); R[:, 2, 2] = one - two * (x * x + y * y)
    return R


def _configuration(links, quat, q, scale, f):
    """per link: frame E (n, 3, 3), origin r (n, 3) relative to the root origin, world joint axis a (n, 3), mass m (n,), centre of mass
    c (n, 3) relative to the root origin, inertia about it in world axes I (n, 3, 3)"""
    n = quat.shape[0]
    nl = len(links)
    E, r, a, m, c, I = ([None] * nl for _ in range(6))
    eye = np.eye(3, dtype=f)
    for i, L in enumerate(links):
        if i == 0:
            E[0], r[0] = _quat_to_mat(quat, f), np.zeros((n, 3), f)
        else:
            p = L["parent"]
            ax = np.asarray(L["axis"], f)
            K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]], f)
            th = q[:, i - 1][:, None, None]
            r[i] = r[p] + _mv(E[p], np.asarray(L["xyz"], f))
            a[i] = _mv(E[p], ax)
            E[i] = E[p] @ (eye + np.sin(th) * K + (f(1) - np.cos(th)) * (K @ K))
        m[i] = f(L["mass"]) * scale[:, i]
        c[i] = r[i] + _mv(E[i], np.asarray(L["com"], f))
        xx, yy, zz, xy, xz, yz = [f(v) for v in L["inertia"]]
        Il = np.array([[xx, xy, xz], [xy, yy, yz], [xz, yz, zz]], f)[None] * scale[:, i][:, None, None]
        I[i] = E[i] @ Il @ np.swapaxes(E[i], -1, -2)
    return E, r, a, m, c, I


def _velocities(links, r, a, c, lin, ang, qd):
    """per link: angular velocity w (n, 3) and the velocity v (n, 3) of the link's centre of mass, for the root's velocity (lin, ang)
    and the joint rates qd"""
    nl = len(links)
    w, vo, v = [None] * nl, [None] * nl, [None] * nl
    for i, L in enumerate(links):
        if i == 0:
            w[0], vo[0] = ang, lin
        else:
            p = L["parent"]
            vo[i] = vo[p] + np.cross(w[p], r[i] - r[p])            # the joint's origin rides on the parent
            w[i] = w[p] + a[i] * qd[:, i - 1][:, None]
        v[i] = vo[i] + np.cross(w[i], c[i] - r[i])
    return w, v


def _momentum(m, c, I, w, v, com, f):
    """(linear momentum, angular momentum about `com`, angular momentum about the root origin), each (n, 3)"""
    P, LG, LO = (np.zeros_like(com) for _ in range(3))
    for i in range(len(m)):
        mv = m[i][:, None] * v[i]
        Iw = _mv(I[i], w[i])
        P = P + mv
        LG = LG + (Iw + np.cross(c[i] - com, mv))
        LO = LO + (Iw + np.cross(c[i], mv))
    return P, LG, LO


def cm_ref(model, state, mass_scale, gravity, dtype=np.float64, armature=0.0, mutate=None):
    """state = (root (n, 13) ROOT_STATE rows of the robot, dof (n, 18, 2)); mass_scale (n, 19) or None; gravity (3,) or (n, 3).
    mutate: a function applied to the list of link dicts first (the sensitivity checks).
    -> dict(state (n, 16), matrix (n, 6, 24), L_root (n, 3): the angular momentum about the root origin), all in `dtype`"""
    f = dtype
    links = copy.deepcopy(model["links"])
    if mutate is not None:
        mutate(links)
    root, dof = np.asarray(state[0], f), np.asarray(state[1], f)
    n, nl = root.shape[0], len(links)
    scale = np.ones((n, nl), f) if mass_scale is None else np.asarray(mass_scale, f)
    g = np.broadcast_to(np.asarray(gravity, f), (n, 3))
    q, qd = dof[:, :, 0], dof[:, :, 1]
    E, r, a, m, c, I = _configuration(links, root[:, 3:7], q, scale, f)
    mass = np.zeros(n, f)
    mc = np.zeros((n, 3), f)
    for i in range(nl):
        mass = mass + m[i]
        mc = mc + m[i][:, None] * c[i]
    com = mc / mass[:, None]
    w, v = _velocities(links, r, a, c, root[:, 7:10], root[:, 10:13], qd)
    P, LG, LO = _momentum(m, c, I, w, v, com, f)
    ke = np.zeros(n, f)
    for i in range(nl):
        ke = ke + f(0.5) * (m[i] * np.sum(v[i] * v[i], axis=1) + np.sum(w[i] * _mv(I[i], w[i]), axis=1))
    ke = ke + f(0.5) * f(armature) * np.sum(qd * qd, axis=1)
    world = root[:, 0:3] + com
    out = np.zeros((n, CM_WORDS), f)
    out[:, 0:3], out[:, 3:6], out[:, 6:9], out[:, 9:12] = world, P / mass[:, None], P, LG
    out[:, CM_MASS], out[:, CM_KINETIC], out[:, CM_POTENTIAL] = mass, ke, -mass * np.sum(g * world, axis=1)
    A = np.zeros((n, 6, NG), f)
    for k in range(NG):
        lin, ang, rate = np.zeros((n, 3), f), np.zeros((n, 3), f), np.zeros((n, NG - 6), f)
        if k < 3:
            lin[:, k] = 1
        elif k < 6:
            ang[:, k - 3] = 1
        else:
            rate[:, k - 6] = 1
        wk, vk = _velocities(links, r, a, c, lin, ang, rate)
        A[:, 0:3, k], A[:, 3:6, k], _ = _momentum(m, c, I, wk, vk, com, f)
    assert out.dtype == f and A.dtype == f and LO.dtype == f
    return dict(state=out, matrix=A, L_root=LO)


def centroidal_states(n, seed=31):
    """the states of tests/state_sets.generate_states (seams, joint limits, random roots; |w| up to 10 rad/s, |qd| up to
    20 rad/s) with the root a few metres from the origin, so that COM carries a real offset without drowning it: fp32 (n, 13), (n, 18, 2)"""
    root, dof, _ = generate_states(n)
    rng = np.random.default_rng(seed)
    root = root.copy()
    root[:, 0:2] = rng.uniform(-3, 3, (n, 2))
    root[:, 2] = rng.uniform(0.2, 2, n)
    return root.astype(np.float32), dof.astype(np.float32)
