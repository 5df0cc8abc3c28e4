"""The state sets the dynamics tests are evaluated on, the fp64 references that share nothing with the kernels, and the error helpers.

  generate_states(n)   -> fp32 root states (n, 13), DOF states (n, 18, 2) and the case of every env: uniformly random SO(3) roots
                          with both quaternion signs, the seams of mat_to_quat's four branches, joints over their whole range (some
                          exactly at a limit), joint speeds to +-20 rad/s, root twists to +-10 rad/s / +-3 m/s, |x|, |y| to 100 m.
  fd_reference(...)    -> fp64 body poses and velocities of the default asset from tests/urdf_independent.kinematics (the URDF
                          fixture, not the model tables).  Quaternions are products of the joints' axis-angle quaternions; velocities
                          are central differences of that FK along the state's own velocity (q + t qd, p0 + t v0, R(t) = exp(t[w]) R0),
                          w = vee(dR/dt R^T).  This shares nothing with the kernel's or the oracle's spatial-velocity code.
  oracle_rows(...)     -> the CPU oracle's rigid-body rows (fp64 or fp32 build) on such states.

tests/test_state_tensors_cpu.py asserts what the set reaches and that the references agree."""
import numpy as np

from tests import urdf_independent as U

BODIES = U.load_fixture()
NB = len(BODIES)   # 21 robot bodies, Isaac order (= the rigid-body rows of the default asset)
DOF_LOWER = np.array([B["lower"] for B in BODIES if B["type"] == "revolute"], np.float64)
DOF_UPPER = np.array([B["upper"] for B in BODIES if B["type"] == "revolute"], np.float64)
FD_H = 1e-5

# ---------------------------------------------------------------- quaternions (xyzw)


def qmul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz])


def axis_angle(axis, ang):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    return np.concatenate([a * np.sin(ang / 2), [np.cos(ang / 2)]])


def quat_mat(q):
    """the rotation matrix formula of the kernels and the oracle (quat_to_mat), also for the not-quite-unit fp32 inputs"""
    return U._quat_R(q)


def _expm_skew(w, t):
    th = np.linalg.norm(w) * t
    if th == 0.0:
        return np.eye(3)
    return U._rot(w, th)


def _vee(W):
    return 0.5 * np.array([W[2, 1] - W[1, 2], W[0, 2] - W[2, 0], W[1, 0] - W[0, 1]])


# ---------------------------------------------------------------- the state set


def _seam_quats():
    """(name, xyzw) at mat_to_quat's branch seams; every one is also given negated"""
    r2 = 1 / np.sqrt(2)
    seams = [("identity", [0, 0, 0, 1]),
             ("pi_x", [1, 0, 0, 0]), ("pi_y", [0, 1, 0, 0]), ("pi_z", [0, 0, 1, 0]),
             ("pi_xy_m00=m11", [r2, r2, 0, 0]), ("pi_xz_m00=m22", [r2, 0, r2, 0]), ("pi_yz_m11=m22", [0, r2, r2, 0])]
    for name, ax in (("x", [1, 0, 0]), ("y", [0, 1, 0]), ("z", [0, 0, 1]), ("111", [1, 1, 1]), ("1-11", [1, -1, 1]),
                     ("-1-11", [-1, -1, 1]), ("0.3,-0.5,0.8", [0.3, -0.5, 0.8])):
        seams.append(("2pi/3_" + name + "_trace=0", axis_angle(ax, 2 * np.pi / 3)))
    rng = np.random.default_rng(11)
    for k in range(6):
        a = rng.normal(size=3)
        seams.append(("w=0_random_axis_%d" % k, np.concatenate([a / np.linalg.norm(a), [0.0]])))
    out = []
    for name, q in seams:
        q = np.asarray(q, np.float64)
        out.append((name, q))
        out.append((name + "_neg", -q))
    return out


def generate_states(n=300, seed=0):
    """fp32 root states (n, 13) [pos, quat xyzw, lin, ang], DOF states (n, 18, 2) [q, qd], and the case of every env.
    The first envs are the seams (with joints at zero, so every body sits on the seam, and with random joints); then joints at a
    limit; then uniformly random roots, each followed by the same state with the quaternion negated."""
    rng = np.random.default_rng(seed)
    root = np.zeros((n, 13), np.float64)
    dof = np.zeros((n, 18, 2), np.float64)
    cases = []
    seams = _seam_quats()
    i = 0

    def rand_twist(e):
        root[e, 0:2] = rng.uniform(-100, 100, 2)
        root[e, 2] = rng.uniform(-1, 2)
        root[e, 7:10] = rng.uniform(-3, 3, 3)
        root[e, 10:13] = rng.uniform(-10, 10, 3)
        dof[e, :, 1] = rng.uniform(-20, 20, 18)

    for name, q in seams:                               # seam, joints at zero: every body rotation equals the root's
        if i >= n:
            break
        rand_twist(i)
        root[i, 3:7] = q
        cases.append("seam:" + name + ":joints_zero")
        i += 1
    for name, q in seams[::2]:                          # seam root, random joints
        if i >= n:
            break
        rand_twist(i)
        root[i, 3:7] = q
        dof[i, :, 0] = rng.uniform(DOF_LOWER, DOF_UPPER)
        cases.append("seam:" + name + ":joints_random")
        i += 1
    for k in range(16):                                 # joints exactly at a limit (the fp32 value of the model's limit)
        if i >= n:
            break
        rand_twist(i)
        qr = rng.normal(size=4)
        root[i, 3:7] = qr / np.linalg.norm(qr)
        at = rng.integers(0, 3, 18)
        dof[i, :, 0] = np.where(at == 0, DOF_LOWER, np.where(at == 1, DOF_UPPER, rng.uniform(DOF_LOWER, DOF_UPPER)))
        cases.append("joint_limits")
        i += 1
    while i < n:                                        # uniformly random SO(3) (normalised 4-d normal), then its negation
        rand_twist(i)
        qr = rng.normal(size=4)
        root[i, 3:7] = qr / np.linalg.norm(qr)
        dof[i, :, 0] = rng.uniform(DOF_LOWER, DOF_UPPER)
        cases.append("random_so3")
        i += 1
        if i < n:
            root[i], dof[i] = root[i - 1], dof[i - 1]
            root[i, 3:7] = -root[i - 1, 3:7]
            cases.append("random_so3_neg")
            i += 1
    return root.astype(np.float32), dof.astype(np.float32), cases


def ball_states(n, seed=1):
    """fp32 (n, 13) ball rows for the kick layout (copied through verbatim by the refresh)"""
    rng = np.random.default_rng(seed)
    b = np.zeros((n, 13))
    b[:, 0:2] = rng.uniform(-100, 100, (n, 2)); b[:, 2] = rng.uniform(0, 1, n)
    qb = rng.normal(size=(n, 4)); b[:, 3:7] = qb / np.linalg.norm(qb, axis=1, keepdims=True)
    b[:, 7:10] = rng.uniform(-3, 3, (n, 3)); b[:, 10:13] = rng.uniform(-10, 10, (n, 3))
    return b.astype(np.float32)


# ---------------------------------------------------------------- the fp64 FD reference (default asset)

def _parents_dofs():
    dofs, k = [], 0
    for B in BODIES:
        dofs.append(k if B["type"] == "revolute" else -1)
        k += B["type"] == "revolute"
    return [B["parent"] for B in BODIES], dofs


_PARENT, _DOF = _parents_dofs()


def _relative_fk(q):
    """body rotations / origins relative to the root frame (root at the origin, unrotated), from the URDF fixture"""
    R, p, _, _ = U.kinematics(BODIES, np.zeros(3), np.array([0.0, 0.0, 0.0, 1.0]), q)
    return np.array(R), np.array(p)


def _relative_quats(q):
    """body orientations relative to the root as products of the joints' axis-angle quaternions (joint frames are unrotated)"""
    out = [None] * NB
    for b, B in enumerate(BODIES):
        if B["parent"] < 0:
            out[b] = np.array([0.0, 0.0, 0.0, 1.0])
        elif _DOF[b] >= 0:
            out[b] = qmul(out[B["parent"]], axis_angle(B["axis"], q[_DOF[b]]))
        else:
            out[b] = out[B["parent"]]
    return np.array(out)


def fd_reference(root, dof):
    """fp64 rigid-body rows (n, 21, 13) of the default asset for fp32 states (root (n, 13), dof (n, 18, 2)): origin position, unit
    quaternion (xyzw), origin velocity, angular velocity -- the last two by a fourth-order central difference (step FD_H) of the FK
    along the state's velocity."""
    root = np.asarray(root, np.float64)
    dof = np.asarray(dof, np.float64)
    n = root.shape[0]
    out = np.zeros((n, NB, 13))
    steps = (-2, -1, 1, 2)
    wts = np.array([1.0, -8.0, 8.0, -1.0]) / (12.0 * FD_H)
    for e in range(n):
        p0, q0, v0, w0 = root[e, 0:3], root[e, 3:7], root[e, 7:10], root[e, 10:13]
        qj, qdj = dof[e, :, 0], dof[e, :, 1]
        R0 = quat_mat(q0)
        Rr, pr = _relative_fk(qj)
        out[e, :, 0:3] = p0 + pr @ R0.T
        qw = np.array([qmul(q0, qr) for qr in _relative_quats(qj)])
        out[e, :, 3:7] = qw / np.linalg.norm(qw, axis=1, keepdims=True)
        dx = np.zeros((NB, 3))
        dR = np.zeros((NB, 3, 3))
        for s, wgt in zip(steps, wts):
            t = s * FD_H
            Rt = _expm_skew(w0, t) @ R0
            Rr_t, pr_t = _relative_fk(qj + t * qdj)
            dx += wgt * (pr_t @ Rt.T)          # the root origin's own motion p0 + t v0 is added exactly below
            dR += wgt * np.einsum("ij,bjk->bik", Rt, Rr_t)
        out[e, :, 7:10] = v0 + dx
        Rb = np.einsum("ij,bjk->bik", R0, Rr)
        out[e, :, 10:13] = np.array([_vee(dR[b] @ Rb[b].T) for b in range(NB)])
    return out


# ---------------------------------------------------------------- comparison helpers

def ulp32(x):
    """the fp32 spacing at |x| (elementwise)"""
    return np.spacing(np.abs(np.asarray(x, np.float32))).astype(np.float64)


def align_quat(q, ref):
    """q (..., 4) with the sign that best matches ref"""
    s = np.sign(np.sum(np.asarray(q, np.float64) * np.asarray(ref, np.float64), axis=-1, keepdims=True))
    return np.asarray(q, np.float64) * np.where(s == 0, 1.0, s)


FIELDS = (("pos", slice(0, 3)), ("quat", slice(3, 7)), ("lin", slice(7, 10)), ("ang", slice(10, 13)))


def field_errors(rows, ref):
    """{field: |rows - ref| elementwise (quaternions sign-aligned)} for (..., 13) body rows"""
    rows = np.asarray(rows, np.float64)
    out = {}
    for name, sl in FIELDS:
        a = align_quat(rows[..., sl], ref[..., sl]) if name == "quat" else rows[..., sl]
        out[name] = np.abs(a - ref[..., sl])
    return out


def oracle_rows(cfg, precision, root, dof, ball=None):
    """rigid-body rows of the CPU oracle (fp64 or fp32 build) for fp32 states root (n, 13), dof (n, 18, 2), ball (n, 13) -> (n, nbe, 13)"""
    from oracle.bez_oracle import Oracle
    n = root.shape[0]
    o = Oracle(cfg, precision=precision)
    for e in range(n):
        r = root[e].astype(np.float64)
        o.set_env_state_f64(e, r[0:3], r[3:7], r[7:10], r[10:13], dof[e, :, 0].astype(np.float64), dof[e, :, 1].astype(np.float64))
    if o.nact == 2 and ball is not None:   # the ball row: through the Isaac root tensor
        rs = o.root_states.reshape(n, 2, 13)
        rs[:, 1] = ball
        o.set_root_states(rs.reshape(-1, 13))
    return o.rigid_body_states.reshape(n, o.nbe, 13)
