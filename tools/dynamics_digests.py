#!/usr/bin/env python3
"""SHA-256 digests of what the dynamics queries write, on the seeded states, udot and parameter rows of the GPU tests
(tests.gpu_util._prepared: generate_states through _write_states).  Two builds that print the same lines compute the same bits:

  BEZ_SIM_LIB=build_ab/parent.so python tools/dynamics_digests.py        (one process per library; profiles/dynamics_refactor_digests.txt, profiles/dynamics_chains_digests.txt)

One line per asset x task x parameters (the defaults; random BEZ_PARAM_MASS_SCALE and BEZ_PARAM_GRAVITY rows) x num_envs: RIGID_BODY_STATE;
the Jacobian and the mass matrix each refreshed alone, then both in one launch; inverse_dynamics for ID_ALL, ID_INERTIA, ID_VELOCITY and
ID_GRAVITY, centroidal (state, matrix) and body_accelerations for ACC_UDOT, ACC_VELOCITY, ACC_GRAVITY, ACC_MOTION (world axes) and ACC_ALL
(the bodies' frames), each into 16-byte aligned buffers and into views 4 bytes off (the kernels' scalar path).  A library without
bez_sim_body_accelerations (BEZ_SIM_LIB naming an older build) prints no acc_* entries, one without bez_sim_generalized_forces no gf_*
entries (wrenches on every body; ENV with points, LOCAL with points, NULL positions at the centres of mass and at the origins), one
without bez_sim_limb_ik no ik_* entries (q and errors for 0, 1 and 8 iterations, ENV and ROOT targets, offsets, with and without a step
limit), one without bez_sim_proximity no prox_* entries (the ground, ball and pair rows), one without bez_sim_forward_dynamics no fd_*
entries (a seeded random force row: floating base with all bias, fixed base, the plain mass solve with bias = 0)."""
import hashlib
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import bez_isaacgym_amd   # noqa: E402,F401  (before anything initialises HIP: DESIGN.md 6.2)
import torch   # noqa: E402

from bez_isaacgym_amd import abi   # noqa: E402
from tests.gpu_util import ASSETS, _prepared   # noqa: E402
from tests.sim_cfg import make_cfg   # noqa: E402

SIZES = (1, 15, 16, 17, 65, 300)
NG = abi.NUM_GEN


def digest(*tensors):
    torch.cuda.synchronize()
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()[:16]


def off4(shape):
    """a contiguous float32 view of `shape` that starts 4 bytes past a 16-byte aligned address"""
    return torch.zeros(torch.Size(shape).numel() + 1, device="cuda:0")[1:].view(shape)


def inverse_dynamics(sim, n, udot, make):
    u, out = make((n, NG)), make((n, NG))
    u.copy_(udot)
    return [sim.inverse_dynamics(u, terms, out).clone() for terms in (abi.ID_ALL, abi.ID_INERTIA, abi.ID_VELOCITY, abi.ID_GRAVITY)]


def centroidal(sim, n, udot, make):
    return sim.centroidal(make((n, abi.CM_WORDS)), make((n, 6, NG)))


def body_accelerations(sim, n, udot, make):
    nb = sim.num_bodies - (1 if sim.has_ball else 0)
    u, out = make((n, NG)), make((n, nb, 6))
    u.copy_(udot)
    return [sim.body_accelerations(u, terms, space, out).clone() for terms, space in
            ((abi.ACC_UDOT, "env"), (abi.ACC_VELOCITY, "env"), (abi.ACC_GRAVITY, "env"), (abi.ACC_MOTION, "env"), (abi.ACC_ALL, "local"))]


def generalized_forces(sim, n, udot, make):
    gen = torch.Generator().manual_seed(11)
    rows = []
    for lo, hi in ((-10.0, 10.0), (-1.0, 1.0), (-0.1, 0.1)):
        t = make((n, sim.num_bodies, 3))
        t.copy_(torch.rand(n, sim.num_bodies, 3, generator=gen) * (hi - lo) + lo)
        rows.append(t)
    out = make((n, NG))
    return [sim.generalized_forces(rows[0], rows[1], x, space, at, out).clone() for x, space, at in
            ((rows[2], "env", "com"), (rows[2], "local", "com"), (None, "env", "com"), (None, "local", "origin"))]


def limb_ik(sim, n, udot, make):
    gen = torch.Generator().manual_seed(13)
    t, q, e = make((n, abi.IK_CHAINS, 7)), make((n, abi.NUM_DOFS)), make((n, abi.IK_CHAINS, 6))
    t.copy_(torch.rand(n, abi.IK_CHAINS, 7, generator=gen) * 0.6 - 0.3)
    w, off = [[1.0, 0.25]] * abi.IK_CHAINS, [[0.01, -0.02, 0.03]] * abi.IK_CHAINS
    return [x.clone() for iters, space, step in ((0, "env", 0.0), (1, "root", 0.0), (8, "env", 0.1), (8, "root", 0.1))
            for x in sim.limb_ik(t, w, off, 0.05, step, iters, space, q, e)]


def proximity(sim, n, udot, make):
    return sim.proximity(make((n, abi.PROX_GROUND_ROWS, 3)), make((n, abi.PROX_BOXES, abi.PROX_WORDS)), make((n, abi.PROX_PAIRS, abi.PROX_WORDS)))


def forward_dynamics(sim, n, udot, make):
    gen = torch.Generator().manual_seed(17)
    f, out = make((n, NG)), make((n, NG))
    f.copy_(torch.rand(n, NG, generator=gen) * 2.0 - 1.0)
    return [sim.forward_dynamics(f, bias, fixed, out).clone() for bias, fixed in
            ((abi.ID_VELOCITY | abi.ID_GRAVITY, False), (abi.ID_VELOCITY | abi.ID_GRAVITY, True), (0, False))]


# (symbol a library must export for the entry to be printed, the entry's prefix, what to digest)
QUERIES = (("bez_sim_inverse_dynamics", "id_", inverse_dynamics), ("bez_sim_centroidal", "cm_", centroidal),
           ("bez_sim_body_accelerations", "acc_", body_accelerations), ("bez_sim_generalized_forces", "gf_", generalized_forces),
           ("bez_sim_limb_ik", "ik_", limb_ik), ("bez_sim_proximity", "prox_", proximity), ("bez_sim_forward_dynamics", "fd_", forward_dynamics))


def main():
    for asset in ASSETS:
        for task in ("bez_kick", "bez_walk"):
            for params in ("default", "random"):
                for n in SIZES:
                    sim, udot = _prepared(make_cfg(n, task=task, seed=5, **ASSETS[asset]), n, params == "random")
                    d = {"rigid_body": digest(sim.refresh(abi.TENSOR_RIGID_BODY_STATE))}
                    J, M = sim.dynamics_tensor("jacobian"), sim.dynamics_tensor("mass_matrix")
                    for name, which, bufs in (("jacobian", "jacobian", (J,)), ("mass_matrix", "mass_matrix", (M,)), ("both", None, (J, M))):
                        for b in bufs:
                            b.fill_(-1.0)
                        sim.refresh_dynamics_tensors(which)
                        d[name] = digest(*bufs)
                    for symbol, prefix, query in QUERIES:
                        if not hasattr(sim.lib, symbol):
                            continue
                        for where, make in (("aligned", lambda shape: torch.zeros(shape, device="cuda:0")), ("offset", off4)):
                            d[prefix + where] = digest(*query(sim, n, udot, make))
                    sim.close()
                    print("%-7s %-8s %-7s n=%-3d %s" % (asset, task, params, n, " ".join("%s=%s" % kv for kv in d.items())), flush=True)


if __name__ == "__main__":
    main()
