"""Reference for bez_sim_generalized_forces (include/bez_sim.h "Generalised forces"): Q = sum over bodies of J_b^T w_b in the generalised
velocity u = [root_lin(3), root_ang(3), qd(18)], rows [total force; total moment about the root origin; joint torques].  Test-only.

  gf_ref   per BODY, in LINK-LOCAL coordinates with Pluecker transforms (the formulation of tests/rbd_numpy, on the helpers of
           tests/inverse_dynamics_numpy.py): the body's wrench is written as the spatial force [n; f] of its link about the LINK's origin
           (f in the link's frame, n = t + p x f with p the point of application in the link's frame), then walked up the body's own path
           to the root: tau_j = S_j . F, F <- Xup_j^T F, and what arrives at the base is turned to world axes.  Every body takes its own
           walk: nothing is summed per link on the way.  A different formulation from the HIP kernel's (world axes about the root origin,
           one summed wrench per link).
  dtype=np.float64 is the reference; the same code in np.float32 is the yardstick of fp32 rounding for the GPU bars (yardstick_error).
  A body whose force and torque rows are all zero is skipped whatever its position row holds (a NaN is not zero); the ball's row, if the
  tensors have one, is never read.  The quaternion is used as it is given (not renormalised), as the kernels use it."""
import numpy as np

from tests import dynamics_numpy as D
from tests.inverse_dynamics_numpy import _T, _mv, _plux, _quat_to_mat, _skew

SPACE_ENV, SPACE_LOCAL = 0, 1
NG = 24
BLOCKS = (("force", slice(0, 3)), ("moment", slice(3, 6)), ("joints", slice(6, NG)))
MUTATIONS = ("offset_ignored", "local_as_env")


def model_of(asset):
    return D.model_of(asset)


def _rows(a, n, nb, f):
    """(n*B, 3) or (n, B, 3) or None -> the robot's rows (n, nb, 3) in `f`, or None"""
    if a is None:
        return None
    a = np.asarray(a)
    return a.reshape(n, -1, 3)[:, :nb].astype(f)


def gf_ref(model, root, dof, forces=None, torques=None, positions=None, space=SPACE_ENV, at="com", dtype=np.float64, mutate=None):
    """root (n, 13) ROOT_STATE rows of the robot, dof (n, 18, 2); forces / torques / positions (n*B, 3) or (n, B, 3) or None, B >= the
    model's bodies (a trailing ball row is ignored) -> (n, 24) in `dtype`.  at: "com" / "origin", the point of application when positions
    is None.  mutate: one of MUTATIONS, the slips the sensitivity check plants."""
    f = dtype
    assert at in ("com", "origin") and space in (SPACE_ENV, SPACE_LOCAL)
    root, dof = np.asarray(root, f), np.asarray(dof, f)
    n = root.shape[0]
    links = model["links"]
    nl, nb = len(links), len(model["body_link"])
    F, T, X = _rows(forces, n, nb, f), _rows(torques, n, nb, f), _rows(positions, n, nb, f)
    zero = np.zeros((n, nb, 3), f)
    loaded = ((F if F is not None else zero) != 0).any(axis=2) | ((T if T is not None else zero) != 0).any(axis=2)   # (a NaN is != 0)
    F = zero if F is None else F
    T = zero if T is None else T
    q = dof[:, :, 0]
    eye = np.eye(3, dtype=f)
    Rw, rw, Xup, S = [None] * nl, [None] * nl, [None] * nl, [None] * nl
    Rw[0] = _quat_to_mat(root[:, 3:7], f)
    rw[0] = np.zeros((n, 3), f)
    for i in range(1, nl):
        L = links[i]
        p = L["parent"]
        K = _skew(np.asarray(L["axis"], f), f)
        th = q[:, i - 1][:, None, None]
        Rj = eye + np.sin(th) * K + (f(1) - np.cos(th)) * (K @ K)
        Xup[i] = _plux(_T(Rj), np.zeros(3, f), f) @ _plux(eye, np.asarray(L["xyz"], f), f)
        S[i] = np.concatenate([np.asarray(L["axis"], f), np.zeros(3, f)])
        Rw[i] = Rw[p] @ Rj
        rw[i] = rw[p] + _mv(Rw[p], np.broadcast_to(np.asarray(L["xyz"], f), (n, 3)))
    local = space == SPACE_LOCAL and mutate != "local_as_env"
    base = np.zeros((n, 6), f)
    tau = np.zeros((n, nl - 1), f)
    for b, l in enumerate(model["body_link"]):
        off = np.zeros(3, f) if mutate == "offset_ignored" else np.asarray(model["body_offset"][b], f)
        com = np.zeros(3, f) if mutate == "offset_ignored" else np.asarray(model["body_com"][b], f)
        # force, torque and point of application in the link's frame, the point relative to the link's origin
        if local:
            fl, tl = F[:, b], T[:, b]
        else:
            fl, tl = _mv(_T(Rw[l]), F[:, b]), _mv(_T(Rw[l]), T[:, b])
        if X is None:
            pl = np.broadcast_to(off if at == "origin" else off + com, (n, 3))
        elif local:
            pl = off + X[:, b]
        else:
            pl = _mv(_T(Rw[l]), X[:, b] - root[:, 0:3] - rw[l])
        on = loaded[:, b]
        if not on.any():
            continue
        W = np.concatenate([tl + np.cross(pl, fl), fl], axis=1)
        W = np.where(on[:, None], W, f(0))
        j = l
        while j > 0:
            tau[:, j - 1] = tau[:, j - 1] + W @ S[j]
            W = _mv(_T(Xup[j]), W)
            j = links[j]["parent"]
        base = base + W
    out = np.concatenate([_mv(Rw[0], base[:, 3:6]), _mv(Rw[0], base[:, 0:3]), tau], axis=1)
    assert out.dtype == f
    return out


def yardstick_error(ref64, *args, **kw):
    """(3,) per block (rows 0:3, 3:6, 6:24): the worst absolute error against ref64 of gf_ref evaluated in np.float32 on the same inputs"""
    r32 = gf_ref(*args, dtype=np.float32, **kw).astype(np.float64)
    return np.array([float(np.abs(r32[:, sl] - ref64[:, sl]).max()) for _, sl in BLOCKS])


def body_velocities(model, root, dof):
    """(n, nb, 6) fp64 [velocity of the body's origin; angular velocity] and (n, nb, 3, 3) body rotations, (n, nb, 3) body origins relative
    to the root origin: an independent forward-kinematics pass in world axes (velocities added up link by link, no Jacobian)"""
    root, dof = np.asarray(root, np.float64), np.asarray(dof, np.float64)
    n = root.shape[0]
    links = model["links"]
    nl = len(links)
    E, r, w, v = [None] * nl, [None] * nl, [None] * nl, [None] * nl   # v: the velocity of the link's ORIGIN
    E[0] = _quat_to_mat(root[:, 3:7], np.float64)
    r[0] = np.zeros((n, 3))
    v[0], w[0] = root[:, 7:10], root[:, 10:13]
    for i in range(1, nl):
        L = links[i]
        p = L["parent"]
        K = _skew(np.asarray(L["axis"], np.float64), np.float64)
        th = dof[:, i - 1, 0][:, None, None]
        d = _mv(E[p], np.broadcast_to(np.asarray(L["xyz"], np.float64), (n, 3)))
        r[i] = r[p] + d
        v[i] = v[p] + np.cross(w[p], d)
        w[i] = w[p] + _mv(E[p], np.broadcast_to(np.asarray(L["axis"], np.float64), (n, 3))) * dof[:, i - 1, 1][:, None]
        E[i] = E[p] @ (np.eye(3) + np.sin(th) * K + (1.0 - np.cos(th)) * (K @ K))
    nb = len(model["body_link"])
    vel, rot, pos = np.zeros((n, nb, 6)), np.zeros((n, nb, 3, 3)), np.zeros((n, nb, 3))
    for b, (l, o) in enumerate(zip(model["body_link"], model["body_offset"])):
        d = _mv(E[l], np.broadcast_to(np.asarray(o, np.float64), (n, 3)))
        pos[:, b] = r[l] + d
        vel[:, b, 0:3] = v[l] + np.cross(w[l], d)
        vel[:, b, 3:6] = w[l]
        rot[:, b] = E[l]
    return vel, rot, pos


def loading(kind, model, root, dof, nbe, space, seed=41):
    """(forces, torques, positions), each (n, nbe, 3) float32 -- nbe the model's bodies plus an optional ball row, which gets random
    numbers too -- for the states root / dof: forces of order 10 N, torques of order 1 N m, points within 0.1 m of the body's origin
    (body frame for SPACE_LOCAL, env coordinates for SPACE_ENV).  kind: "all" every body loaded; "round_robin" body e mod nb alone in env
    e; "feet" both feet only.  Unloaded rows of forces and torques are zero; their position rows stay filled."""
    rng = np.random.default_rng(seed)
    n, nb, names = np.asarray(root).shape[0], len(model["body_link"]), model["body_names"]
    F = rng.uniform(-10, 10, (n, nbe, 3))
    T = rng.uniform(-1, 1, (n, nbe, 3))
    P = rng.uniform(-0.1, 0.1, (n, nbe, 3))
    if space == SPACE_ENV:
        _, rot, pos = body_velocities(model, root, dof)
        P[:, :nb] = np.asarray(root, np.float64)[:, None, 0:3] + pos + _mv(rot, P[:, :nb])
    keep = np.zeros((n, nbe), bool)
    if kind == "all":
        keep[:, :nb] = True
    elif kind == "round_robin":
        keep[np.arange(n), np.arange(n) % nb] = True
    else:
        assert kind == "feet"
        keep[:, [names.index("/left_foot"), names.index("/right_foot")]] = True
    keep[:, nb:] = True   # the ball's row, never read
    F[~keep] = 0
    T[~keep] = 0
    return F.astype(np.float32), T.astype(np.float32), P.astype(np.float32)
