"""The convergence case of the limb inverse kinematics, shared by tests/test_limb_ik_cpu.py and tests/test_gpu_limb_ik.py."""
import numpy as np

from tests import dynamics_numpy as D
from tests import limb_ik_numpy as IK

# the convergence case (shared with the GPU test): lambda for which the fp64 reference's weighted residual after 30 iterations from a
# start in the middle 60 % of every joint's range, towards a pose |delta| <= 0.3 rad away, is below 1e-4 in every env
CONV = dict(n=300, iters=30, damping=0.01, weights=[[1.0, 0.05]] * 5, seed=17, delta=0.3, middle=0.6, bound=1e-4)


def convergence_inputs(model):
    """(root (n, 13) at the origin, q (n, 18) fp32 starts, targets (n, 5, 7) fp32 in the root's frame): reachable by construction"""
    rng = np.random.default_rng(CONV["seed"])
    lo, hi = np.asarray(D.MODEL["dof_lower"]), np.asarray(D.MODEL["dof_upper"])
    mid, half = 0.5 * (lo + hi), 0.5 * (hi - lo) * CONV["middle"]
    n = CONV["n"]
    q = (mid + rng.uniform(-1, 1, (n, 18)) * half).astype(np.float32)
    delta = rng.uniform(-CONV["delta"], CONV["delta"], (n, 18))
    root = np.zeros((n, 13), np.float32)
    root[:, 6] = 1.0
    return root, q, IK.make_targets(model, root, q, delta, IK.SPACE_ROOT)
