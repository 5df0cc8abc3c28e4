"""The reference for bez_sim_operational_space (include/bez_sim.h "Operational space"): the Jacobians J_c of the five controlled frames,
J_c M^-1, the Delassus matrix W = J_E M^-1 J_E^T and Lambda_c = W_cc^-1, put together from what the project already trusts -- the chains'
forward kinematics and Jacobian columns of tests/limb_ik_numpy (chain_fk / jacobian) plus the base block, M from
tests/forward_dynamics_numpy.M_batch -- and a dense np.linalg.solve / np.linalg.inv, every operation in `dtype`.  fp64 is the reference;
the same code in np.float32 is the yardstick of fp32 rounding for the GPU bars.  It knows nothing of the block arrow: the kernel's
elimination is held to it.  Not a test.

  mutate   one of MUTATIONS, the slips the sensitivity check plants: "offset_ignored" (the frames sit at the end bodies' origins),
           "armature_dropped", "mass_scale_dropped", "quirk_ignored" (the joint origin box + cleats moves stays where the model has it),
           "linear_rows_at_body_origin" (the base block is shifted to the controlled point, the joint columns' levers are not)."""
import numpy as np

from tests import dynamics_numpy as D
from tests import forward_dynamics_numpy as FD
from tests import limb_ik_numpy as IK

NCH, NG, NF = 5, 24, 30
MUTATIONS = ("offset_ignored", "armature_dropped", "mass_scale_dropped", "quirk_ignored", "linear_rows_at_body_origin")
OUTPUTS = ("jac", "jminv", "w", "lambda")
LIN, ANG = slice(0, 3), slice(3, 6)


def _quirk_links(links):
    for L in links:
        if L["name"] == "/right_ankle":
            L["xyz"] = list(D.MODEL["box_asset"]["cleats_right_ankle_xyz"])


def _skew(v, f):
    """(n, 3) -> (n, 3, 3)"""
    S = np.zeros(v.shape[:-1] + (3, 3), f)
    S[..., 0, 1], S[..., 0, 2] = -v[..., 2], v[..., 1]
    S[..., 1, 0], S[..., 1, 2] = v[..., 2], -v[..., 0]
    S[..., 2, 0], S[..., 2, 1] = -v[..., 1], v[..., 0]
    return S


def frame_jacobians(model, root, dof, offsets=None, dtype=np.float64, quirk=False, mutate=None):
    """J_E (n, 5, 6, 24) in `dtype`: per chain the controlled frame's [linear; angular] rows in u = [root_lin, root_ang, qd], world axes.
    The root quaternion is used as it is given (as the kernels use it)."""
    f = dtype
    root, dof = np.asarray(root).astype(f), np.asarray(dof).astype(f)
    q = dof[:, :, 0] if dof.ndim == 3 else dof
    n = q.shape[0]
    off = np.zeros((NCH, 3)) if offsets is None or mutate == "offset_ignored" else np.asarray(offsets, np.float64).reshape(NCH, 3)
    off = off.astype(np.float32)   # the call takes fp32 parameters
    E0 = IK.quat_to_mat(root[:, 3:7], f)
    J = np.zeros((n, NCH, 6, NG), f)
    eye = np.eye(3, dtype=f)
    for c, (first, k) in enumerate(IK.chains(model)):
        qc = q[:, first - 1:first - 1 + k]
        p, _, A, O = IK.chain_fk(model, c, qc, f, quirk, off[c])
        Jcc = IK.jacobian(p, A, O)
        if mutate == "linear_rows_at_body_origin":
            pb, _, Ab, Ob = IK.chain_fk(model, c, qc, f, quirk, None)
            Jcc = IK.jacobian(pb, Ab, Ob)
        x = np.einsum("nij,nj->ni", E0, p)
        J[:, c, LIN, 0:3] = eye
        J[:, c, ANG, 3:6] = eye
        J[:, c, LIN, 3:6] = -_skew(x, f)
        J[:, c, LIN, 5 + first:5 + first + k] = E0 @ Jcc[:, LIN]
        J[:, c, ANG, 5 + first:5 + first + k] = E0 @ Jcc[:, ANG]
    assert J.dtype == f
    return J


def mass_matrices(model, root, dof, scale, armature, dtype=np.float64, quirk=False, mutate=None):
    """(n, 24, 24) in `dtype`: FD.M_batch with the slips of `mutate` and the joint origin box + cleats moves"""
    return FD.M_batch(model, root, dof, None if mutate == "mass_scale_dropped" else scale, 0.0 if mutate == "armature_dropped" else armature,
                      dtype, _quirk_links if quirk and mutate != "quirk_ignored" else None)


def op_space_ref(model, root, dof, offsets=None, scale=None, armature=0.0, fixed_base=False, dtype=np.float64, quirk=False, mutate=None,
                 M=None, want_lambda=True):
    """{"jac" (n, 5, 6, 24), "jminv" (n, 5, 6, 24), "w" (n, 30, 30), "lambda" (n, 5, 6, 6) or None, "minvjt" (n, 24, 30)} in `dtype`.
    root (n, 13) ROOT_STATE rows of the robot, dof (n, 18, 2), offsets (5, 3) or None, scale (n, 19) or None.  fixed_base: M becomes
    M[6:, 6:] (jminv[..., 0:6] = 0, lambda is None).  M: mass_matrices of the same arguments where the caller has it already."""
    f = dtype
    assert mutate is None or mutate in MUTATIONS
    J = frame_jacobians(model, root, dof, offsets, f, quirk and mutate != "quirk_ignored", mutate)
    n = J.shape[0]
    if M is None:
        M = mass_matrices(model, root, dof, scale, armature, f, quirk, mutate)
    assert M.dtype == f
    JE = J.reshape(n, NF, NG)
    lo = 6 if fixed_base else 0
    T = np.zeros((n, NG, NF), f)
    T[:, lo:] = np.linalg.solve(M[:, lo:, lo:], np.swapaxes(JE[:, :, lo:], 1, 2))
    W = JE[:, :, lo:] @ T[:, lo:]
    lam = None
    if want_lambda and not fixed_base:
        lam = np.stack([np.linalg.inv(W[:, 6 * c:6 * c + 6, 6 * c:6 * c + 6]) for c in range(NCH)], axis=1)
        assert lam.dtype == f
    out = {"jac": J, "jminv": np.swapaxes(T, 1, 2).reshape(n, NCH, 6, NG).copy(), "w": W, "lambda": lam, "minvjt": T}
    assert all(v is None or v.dtype == f for v in out.values())
    return out


def classes(fixed_base=False):
    """{class name: (output, boolean mask over one env's elements)}: the unit classes a bar is formed over.  jac: linear / angular rows;
    jminv: linear / angular rows x columns 0:3, 3:6, 6:24; w and lambda: lin-lin, lin-ang, ang-ang.  With a fixed base the classes that
    are zero by structure are left out (they are checked to the bit)."""
    lin5 = np.zeros((NCH, 6), bool); lin5[:, LIN] = True
    out = {}
    for name, rows in (("lin", lin5), ("ang", ~lin5)):
        out["jac_" + name] = ("jac", np.broadcast_to(rows[:, :, None], (NCH, 6, NG)).copy())
        for cname, cols in (("base_lin", slice(0, 3)), ("base_ang", slice(3, 6)), ("joints", slice(6, NG))):
            if fixed_base and cname != "joints":
                continue
            m = np.zeros((NCH, 6, NG), bool)
            m[:, :, cols] = True
            out["jminv_%s_%s" % (name, cname)] = ("jminv", m & rows[:, :, None])
    l30 = lin5.reshape(NF)
    pairs = {"lin_lin": l30[:, None] & l30[None, :], "ang_ang": ~l30[:, None] & ~l30[None, :]}
    pairs["lin_ang"] = ~(pairs["lin_lin"] | pairs["ang_ang"])
    blockdiag = np.kron(np.eye(NCH, dtype=bool), np.ones((6, 6), bool))
    for name, m in pairs.items():
        out["w_" + name] = ("w", m & blockdiag if fixed_base else m)
        if not fixed_base:
            out["lambda_" + name] = ("lambda", np.stack([m[6 * c:6 * c + 6, 6 * c:6 * c + 6] for c in range(NCH)]))
    return out


def class_bars(ref64, ref32, fixed_base=False):
    """{class: bar}: 3 x the worst absolute error of the np.float32 evaluation against fp64 in the class + 2 fp32 ulps of the class's
    largest |reference| (the project's convention)"""
    bars = {}
    for name, (o, m) in classes(fixed_base).items():
        r64 = ref64[o][:, m]
        bars[name] = 3.0 * float(np.abs(ref32[o].astype(np.float64)[:, m] - r64).max()) + 2.0 * float(np.spacing(np.float32(np.abs(r64).max())))
    return bars


def class_ratios(got, ref64, bars, fixed_base=False):
    """{class: worst |got - ref64| / bar} over every element of every env; `got`: {output: array or None}, outputs that are None are left out"""
    out = {}
    for name, (o, m) in classes(fixed_base).items():
        if got.get(o) is None:
            continue
        n = got[o].shape[0]
        out[name] = float(np.abs(np.asarray(got[o], np.float64)[:, m] - ref64[o][:n][:, m]).max() / bars[name])
    return out
