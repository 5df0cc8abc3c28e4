"""Reference for bez_sim_limb_ik (include/bez_sim.h "Limb inverse kinematics"): damped least squares on each of the five chains off the
torso, towards a pose of the chain's end body (displaced by an offset), in the root's axes about the root origin.  Test-only; reads only
the model JSON (tests/dynamics_numpy.MODEL).

  limb_ik_ref   per CHAIN, with the chain's own forward kinematics (Rodrigues rotations of the model's axes, the kernels go through
                link_kinematics' column rotations), the Jacobian columns [a x (p - r); a], the normal equations solved by
                numpy.linalg.solve (the kernel: a Cholesky factor in registers), the step limit, the clamp.
  dtype=np.float64 is the reference; the same code in np.float32 is the yardstick of fp32 rounding for the GPU bars (yardstick_error).
  The root quaternion is used as it is given (as the kernels use it); the target quaternion is normalised.
  quirk=True: the box asset with cleats, whose right ankle's joint origin is the model's box_asset.cleats_right_ankle_xyz."""
import numpy as np

from tests import dynamics_numpy as D

SPACE_ENV, SPACE_ROOT = 0, 1
NCH, ND = 5, 18
MUTATIONS = ("offset_ignored", "weight_ignored", "step_limit_ignored", "limit_rows_ignored", "quirk_ignored")
BLOCKS = tuple("q_chain%d" % c for c in range(NCH)) + ("position", "rotation")


def model_of(asset):
    return D.model_of(asset)


def chains(model):
    """[(first link, number of links)] of the chains off the torso, from the links' parents, in the order of their first link"""
    links = model["links"]
    out = []
    for l in range(1, len(links)):
        if links[l]["parent"] == 0:
            out.append([l, 1])
        else:
            assert links[l]["parent"] == l - 1 and out[-1][0] + out[-1][1] == l, "not serial chains off the torso"
            out[-1][1] += 1
    return [tuple(c) for c in out]


def end_body(model, c):
    first, k = chains(model)[c]
    return model["links"][first + k - 1]["body"]


def _skew(a, f):
    return np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]], f)


def _mv(M, v):
    return np.einsum("nij,nj->ni", M, v)


def _T(M):
    return np.swapaxes(M, -1, -2)


def quat_to_mat(q, f):
    """(n, 4) xyzw, used as given -> (n, 3, 3)"""
    x, y, z, w = (q[:, k] for k in range(4))
    one, two = f(1), f(2)
    R = np.empty((q.shape[0], 3, 3), f)
    R[:, 0, 0] = one - two * (y * y + z * z); R[:, 0, 1] = two * (x * y - z * w); R[:, 0, 2] = two * (x * z + y * w)
    R[:, 1, 0] = two * (x * y + z * w); R[:, 1, 1] = one - two * (x * x + z * z); R[:, 1, 2] = two * (y * z - x * w)
    R[:, 2, 0] = two * (x * z - y * w); R[:, 2, 1] = two * (y * z + x * w); R[:, 2, 2] = one - two * (x * x + y * y)
    return R


def mat_to_quat(R, f):
    """(n, 3, 3) rotations -> (n, 4) xyzw: of the four forms, the one whose pivot (w, x, y or z) is largest"""
    m = lambda i, j: R[:, i, j]
    tr = m(0, 0) + m(1, 1) + m(2, 2)
    piv = np.stack([tr, m(0, 0), m(1, 1), m(2, 2)], axis=1)
    k = np.argmax(piv, axis=1)
    one, two, qr = f(1), f(2), f(0.25)
    with np.errstate(invalid="ignore", divide="ignore"):
        s0 = np.sqrt(tr + one) * two
        s1 = np.sqrt(one + m(0, 0) - m(1, 1) - m(2, 2)) * two
        s2 = np.sqrt(one + m(1, 1) - m(0, 0) - m(2, 2)) * two
        s3 = np.sqrt(one + m(2, 2) - m(0, 0) - m(1, 1)) * two
        forms = [np.stack([(m(2, 1) - m(1, 2)) / s0, (m(0, 2) - m(2, 0)) / s0, (m(1, 0) - m(0, 1)) / s0, qr * s0], axis=1),
                 np.stack([qr * s1, (m(0, 1) + m(1, 0)) / s1, (m(0, 2) + m(2, 0)) / s1, (m(2, 1) - m(1, 2)) / s1], axis=1),
                 np.stack([(m(0, 1) + m(1, 0)) / s2, qr * s2, (m(1, 2) + m(2, 1)) / s2, (m(0, 2) - m(2, 0)) / s2], axis=1),
                 np.stack([(m(0, 2) + m(2, 0)) / s3, (m(1, 2) + m(2, 1)) / s3, qr * s3, (m(1, 0) - m(0, 1)) / s3], axis=1)]
    out = np.where((k == 0)[:, None], forms[0], np.where((k == 1)[:, None], forms[1], np.where((k == 2)[:, None], forms[2], forms[3])))
    nan = ~np.isfinite(piv).all(axis=1)
    out[nan] = np.nan
    return out.astype(f)


def chain_fk(model, c, q, dtype=np.float64, quirk=False, offset=None):
    """chain c at the angles q (n, k) -> (p (n, 3), R (n, 3, 3), axes (n, k, 3), joint origins (n, k, 3)), root axes about the root origin;
    p, R: the end body's frame displaced by `offset` (3,) in its own axes"""
    f = dtype
    links = model["links"]
    first, k = chains(model)[c]
    q = np.asarray(q, f)
    n = q.shape[0]
    E = np.broadcast_to(np.eye(3, dtype=f), (n, 3, 3)).copy()
    r = np.zeros((n, 3), f)
    eye = np.eye(3, dtype=f)
    A, O = np.zeros((n, k, 3), f), np.zeros((n, k, 3), f)
    for i in range(k):
        L = links[first + i]
        xyz = np.asarray(L["xyz"], f)
        if quirk and L["name"] == "/right_ankle":
            xyz = np.asarray(D.MODEL["box_asset"]["cleats_right_ankle_xyz"], f)
        axis = np.asarray(L["axis"], f)
        r = r + _mv(E, np.broadcast_to(xyz, (n, 3)))
        A[:, i] = _mv(E, np.broadcast_to(axis, (n, 3)))
        O[:, i] = r
        K = _skew(axis, f)
        th = q[:, i][:, None, None]
        E = E @ (eye + np.sin(th) * K + (f(1) - np.cos(th)) * (K @ K))
    b = links[first + k - 1]["body"]
    tip = np.asarray(model["body_offset"][b], f)
    if offset is not None:
        tip = tip + np.asarray(offset, f)
    p = r + _mv(E, np.broadcast_to(tip, (n, 3)))
    assert p.dtype == f and E.dtype == f
    return p, E, A, O


def pose_error(pd, Rd, p, R, f):
    """(n, 6): [pd - p ; 2 sign(w) (x, y, z)] with (x, y, z, w) the quaternion of Rd R^T, sign(0) = +1"""
    qe = mat_to_quat(Rd @ _T(R), f)
    sg = np.where(qe[:, 3] < 0, f(-2), f(2))
    return np.concatenate([pd - p, sg[:, None] * qe[:, 0:3]], axis=1)


def jacobian(p, A, O):
    """(n, 6, k): columns [a x (p - r); a]"""
    return np.concatenate([np.cross(A, p[:, None, :] - O), A], axis=2).transpose(0, 2, 1)


def targets_in_root(root, targets, space, f):
    """targets (n, 5, 7) -> (pd (n, 5, 3), Rd (n, 5, 3, 3)) in the root's axes about the root origin"""
    t = np.asarray(targets).astype(f)
    n = t.shape[0]
    pd = t[:, :, 0:3].copy()
    with np.errstate(invalid="ignore"):
        qn = t[:, :, 3:7] / np.sqrt((t[:, :, 3:7] ** 2).sum(axis=2, keepdims=True))
    Rd = np.stack([quat_to_mat(qn[:, c], f) for c in range(NCH)], axis=1)
    if space == SPACE_ENV:
        root = np.asarray(root).astype(f)
        E0 = quat_to_mat(root[:, 3:7], f)
        for c in range(NCH):
            pd[:, c] = _mv(_T(E0), pd[:, c] - root[:, 0:3])
            Rd[:, c] = _T(E0) @ Rd[:, c]
    return pd, Rd


def limb_ik_ref(model, root, dof, targets, weights, offsets=None, damping=0.05, max_step=0.0, iters=1, space=SPACE_ENV, lower=None,
                upper=None, dtype=np.float64, quirk=False, mutate=None):
    """root (n, 13), dof (n, 18, 2) or q (n, 18), targets (n, 5, 7), weights (5, 2), offsets (5, 3) or None, lower / upper (n, 18) limit rows
    or None for the model's -> (q (n, 18), err (n, 5, 6)) in `dtype`.  mutate: one of MUTATIONS, the slips the sensitivity check plants."""
    f = dtype
    assert mutate is None or mutate in MUTATIONS
    dof = np.asarray(dof)
    q0 = (dof[:, :, 0] if dof.ndim == 3 else dof).astype(f)
    n = q0.shape[0]
    W = np.asarray(weights, np.float64).reshape(NCH, 2)
    off = np.zeros((NCH, 3)) if offsets is None or mutate == "offset_ignored" else np.asarray(offsets, np.float64).reshape(NCH, 3)
    off = off.astype(np.float32)   # the call takes fp32 parameters
    if mutate == "limit_rows_ignored":
        lower = upper = None
    lo = np.broadcast_to(np.asarray(model.get("dof_lower", D.MODEL["dof_lower"]), np.float64).astype(np.float32), (n, ND)) if lower is None else np.asarray(lower)
    hi = np.broadcast_to(np.asarray(model.get("dof_upper", D.MODEL["dof_upper"]), np.float64).astype(np.float32), (n, ND)) if upper is None else np.asarray(upper)
    lo, hi = lo.astype(f), hi.astype(f)
    if mutate == "step_limit_ignored":
        max_step = 0.0
    quirk = quirk and mutate != "quirk_ignored"
    pd, Rd = targets_in_root(root, targets, space, f)
    lam2 = f(np.float32(damping)) * f(np.float32(damping))
    q_out, err = q0.copy(), np.zeros((n, NCH, 6), f)
    for c, (first, k) in enumerate(chains(model)):
        wp, wr = f(np.float32(W[c, 0])), f(np.float32(W[c, 1]))
        if wp == 0 and wr == 0:
            continue
        if mutate == "weight_ignored":
            wp = wr = f(1)
        d0 = first - 1
        q = q0[:, d0:d0 + k].copy()
        w6 = np.array([wp, wp, wp, wr, wr, wr], f)
        for it in range(iters + 1):
            p, R, A, O = chain_fk(model, c, q, f, quirk, off[c])
            e = pose_error(pd[:, c], Rd[:, c], p, R, f)
            if it == iters:
                break
            J = jacobian(p, A, O)
            JW = _T(J) * w6[None, None, :]
            N = JW @ J + lam2 * np.eye(k, dtype=f)
            b = np.einsum("nkr,nr->nk", JW, e)
            bad = ~(np.isfinite(N).all(axis=(1, 2)) & np.isfinite(b).all(axis=1))
            N[bad] = np.eye(k, dtype=f)
            dq = np.linalg.solve(N, b[:, :, None])[:, :, 0].astype(f)
            dq[bad] = np.nan
            if max_step > 0:
                big = np.abs(dq).max(axis=1)
                with np.errstate(invalid="ignore", divide="ignore"):
                    sc = np.where(big > f(np.float32(max_step)), f(np.float32(max_step)) / big, f(1))
                dq = dq * sc[:, None]
            with np.errstate(invalid="ignore"):
                q = np.clip(q + dq, lo[:, d0:d0 + k], hi[:, d0:d0 + k])
            q[~np.isfinite(dq)] = np.nan
        q_out[:, d0:d0 + k] = q
        err[:, c] = e
    assert q_out.dtype == f and err.dtype == f
    return q_out, err


def block_slices(model):
    """{block name: (which output, index)} -- each chain's q, the position rows, the rotation rows"""
    out = {}
    for c, (first, k) in enumerate(chains(model)):
        out["q_chain%d" % c] = ("q", (slice(None), slice(first - 1, first - 1 + k)))
    out["position"] = ("err", (slice(None), slice(None), slice(0, 3)))
    out["rotation"] = ("err", (slice(None), slice(None), slice(3, 6)))
    return out


def yardstick_error(ref64, *args, **kw):
    """{block: worst absolute error against ref64 = (q, err) of limb_ik_ref evaluated in np.float32 on the same inputs}"""
    q32, e32 = limb_ik_ref(*args, dtype=np.float32, **kw)
    got = {"q": q32.astype(np.float64), "err": e32.astype(np.float64)}
    ref = {"q": ref64[0], "err": ref64[1]}
    return {name: float(np.abs(got[w][ix] - ref[w][ix]).max()) for name, (w, ix) in block_slices(args[0]).items()}


def weighted_residual(err, weights):
    """(n, 5): sqrt(w_pos |e_pos|^2 + w_rot |e_rot|^2) per chain"""
    W = np.asarray(weights, np.float64).reshape(NCH, 2)
    e = np.asarray(err, np.float64)
    return np.sqrt(W[None, :, 0] * (e[:, :, 0:3] ** 2).sum(axis=2) + W[None, :, 1] * (e[:, :, 3:6] ** 2).sum(axis=2))


def make_targets(model, root, q, delta, space, offsets=None, quirk=False, quat_scale=None):
    """fp32 targets (n, 5, 7): the poses (fp64 forward kinematics) of the controlled frames at clip(q + delta) between the model's limits,
    as the space carries them; quat_scale (n,): factors on the quaternions (the call normalises them)"""
    q = np.asarray(q, np.float64)
    n = q.shape[0]
    qt = np.clip(q + delta, np.asarray(D.MODEL["dof_lower"]), np.asarray(D.MODEL["dof_upper"]))
    root = np.asarray(root, np.float64)
    E0 = quat_to_mat(root[:, 3:7], np.float64)
    T = np.zeros((n, NCH, 7))
    for c, (first, k) in enumerate(chains(model)):
        p, R, _, _ = chain_fk(model, c, qt[:, first - 1:first - 1 + k], np.float64, quirk, None if offsets is None else np.asarray(offsets, np.float32)[c])
        if space == SPACE_ENV:
            p, R = root[:, 0:3] + _mv(E0, p), E0 @ R
        T[:, c, 0:3] = p
        T[:, c, 3:7] = mat_to_quat(R, np.float64)
    if quat_scale is not None:
        T[:, :, 3:7] *= np.asarray(quat_scale)[:, None, None]
    return T.astype(np.float32)
