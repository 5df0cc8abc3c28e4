"""Times one of the dynamics queries at num_envs = 4096 beside its yardsticks in the same run.  Prints one JSON line.

  python tools/dynamics_bench.py {tensors,inverse_dynamics,centroidal,body_accelerations,generalized_forces,limb_ik,proximity,forward_dynamics,operational_space} [--num-envs 4096] [--launches 200] [--warmup 20] [--cleats]
  python tools/dynamics_bench.py inverse_dynamics > profiles/inverse_dynamics_bench.json      (the committed records)
  python tools/dynamics_bench.py centroidal > profiles/centroidal_bench.json
  python tools/dynamics_bench.py body_accelerations > profiles/body_accelerations_bench.json
  python tools/dynamics_bench.py generalized_forces > profiles/generalized_forces_bench.json
  python tools/dynamics_bench.py limb_ik > profiles/limb_ik_bench.json
  python tools/dynamics_bench.py proximity > profiles/proximity_bench.json

tensors: bez_sim_refresh_dynamics_tensors (the Jacobian, the mass matrix, both) beside a plain device fill of the same bytes -- the kernel
is store-bound by construction, so the fill (hipMemsetAsync over the very buffer the refresh writes) is its yardstick.
inverse_dynamics: bez_sim_inverse_dynamics (all terms; gravity only) beside refresh_rigid_body_state -- the same per-lane forward
kinematics -- and the route the call replaces: a mass-matrix refresh followed by torch.bmm(M, udot).
centroidal: bez_sim_centroidal (both outputs; the state alone) beside bez_sim_inverse_dynamics with all terms -- the neighbour of the same
shape -- and the route the call replaces: a mass-matrix refresh followed by the torch ops that rebuild the 16 + 144 numbers per env from M
and u (rows 0:6 of M times u, the centre of mass un-skewed from M[0:3, 3:6], the moment shifted to it, 1/2 u^T M u).  The replaced route
is handed u and the root positions ready-made: refreshing them is not counted against it.
body_accelerations: bez_sim_body_accelerations (motion terms in world axes; all terms in the bodies' frames; the bias acceleration alone)
beside refresh_rigid_body_state -- the same per-lane forward kinematics and a read-out of the same kind -- beside bez_sim_inverse_dynamics
with all terms -- whose outward half it is -- and beside the route the call replaces for the UDOT term: a Jacobian refresh followed by
torch.matmul(J, udot).
generalized_forces: bez_sim_generalized_forces (every body loaded, ENV space with points; one body loaded -- the skipped bodies' rows are
still brought into LDS) beside refresh_rigid_body_state, beside bez_sim_inverse_dynamics with all terms -- whose return sweep it is -- and
beside the route the call replaces: a Jacobian refresh followed by torch.einsum of J with the wrenches at the bodies' origins.
limb_ik: bez_sim_limb_ik (all five chains for 1 and 8 iterations; the pose-error query; the two legs alone with a step limit) beside
refresh_rigid_body_state and beside the route the call replaces for ONE iteration: a rigid-body and a Jacobian refresh, the limbs'
columns sliced in torch and torch.linalg.solve per chain (more iterations of that route need the state written back in between).
proximity: bez_sim_proximity (all three outputs; the ground rows alone; the pairs alone) beside refresh_rigid_body_state -- the same
per-lane forward kinematics -- and the route the call replaces: a rigid-body refresh followed by batched torch ops that rebuild the
collision shapes from bez_model.json on the body rows and compute the same 23 + 11 + 28 rows.
forward_dynamics: bez_sim_forward_dynamics (floating base with all bias; fixed base; the plain mass solve) beside bez_sim_inverse_dynamics
with all terms -- whose walk is one of its two front ends -- beside the mass-matrix refresh -- the other -- and the route the call
replaces: a mass-matrix refresh, bez_sim_inverse_dynamics for h and torch.linalg.solve.
operational_space: bez_sim_operational_space (all four outputs, floating base; w alone; the fixed base without lambda) beside
bez_sim_forward_dynamics -- whose factorisation it shares -- and the route the call replaces: a rigid-body, a Jacobian and a mass-matrix
refresh, the five end bodies' rows sliced and their linear rows shifted to the controlled points in torch, torch.linalg.solve on the 24 x 24
systems with 30 right-hand sides, torch.bmm for W (and, counted apart, torch.linalg.inv of the five diagonal blocks for Lambda).

Each figure is the median over --launches (>= 200) single launches, each between its own pair of events on one stream, after --warmup
launches.  Nothing flushes the caches between launches, for a call and its yardsticks alike.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bez_isaacgym_amd import abi  # noqa: E402
from bez_isaacgym_amd.sim import BezSim  # noqa: E402

DEV = "cuda:0"


def timed(fn, launches, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    pairs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(launches)]
    for a, b in pairs:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    us = sorted(a.elapsed_time(b) * 1e3 for a, b in pairs)
    return {"median_us": round(statistics.median(us), 2), "min_us": round(us[0], 2), "p90_us": round(us[int(0.9 * len(us))], 2)}


def tensors(sim, n, t):
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemsetAsync.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p]
    hip.hipMemsetAsync.restype = C.c_int
    sim.step(torch.zeros(n * 18, device=DEV))   # a state off the reset pose
    J, M = sim.dynamics_tensor("jacobian"), sim.dynamics_tensor("mass_matrix")

    def fill(*bufs):
        def run():
            for b in bufs:
                assert hip.hipMemsetAsync(C.c_void_p(b.data_ptr()), 0, b.numel() * 4, C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
        return run

    res = {"bytes": {"jacobian": J.numel() * 4, "mass_matrix": M.numel() * 4}}
    for name, which, bufs in (("jacobian", ["jacobian"], (J,)), ("mass_matrix", ["mass_matrix"], (M,)), ("both", ["jacobian", "mass_matrix"], (J, M))):
        r, f = t(lambda: sim.refresh_dynamics_tensors(which)), t(fill(*bufs))
        nbytes = sum(b.numel() * 4 for b in bufs)
        res[name] = {"refresh": r, "fill": f, "ratio": round(r["median_us"] / f["median_us"], 3),
                     "refresh_GBps": round(nbytes / r["median_us"] / 1e3, 1), "fill_GBps": round(nbytes / f["median_us"] / 1e3, 1)}
    sim.refresh_dynamics_tensors()
    torch.cuda.synchronize()
    assert torch.isfinite(J).all() and torch.isfinite(M).all()
    return res


def inverse_dynamics(sim, n, t):
    sim.step(torch.zeros(n * 18, device=DEV))   # a state off the reset pose
    udot = torch.rand(n, abi.NUM_GEN, device=DEV) * 20 - 10
    out = torch.zeros(n, abi.NUM_GEN, device=DEV)
    M = sim.dynamics_tensor("mass_matrix")
    mu = torch.zeros(n, abi.NUM_GEN, 1, device=DEV)

    def replaced():
        sim.refresh_dynamics_tensors("mass_matrix")
        torch.bmm(M, udot.unsqueeze(2), out=mu)

    res = {"inverse_dynamics_all_terms": t(lambda: sim.inverse_dynamics(udot, abi.ID_ALL, out)),
           "inverse_dynamics_gravity_only": t(lambda: sim.inverse_dynamics(None, abi.ID_GRAVITY, out)),
           "refresh_rigid_body_state": t(lambda: sim.refresh(abi.TENSOR_RIGID_BODY_STATE)),
           "mass_matrix_refresh_plus_bmm": t(replaced)}
    res["ratio_to_rigid_body_refresh"] = round(res["inverse_dynamics_all_terms"]["median_us"] / res["refresh_rigid_body_state"]["median_us"], 3)
    res["ratio_to_replaced_route"] = round(res["inverse_dynamics_all_terms"]["median_us"] / res["mass_matrix_refresh_plus_bmm"]["median_us"], 3)
    # the two routes agree on the inertia term
    sim.inverse_dynamics(udot, abi.ID_INERTIA, out)
    replaced()
    torch.cuda.synchronize()
    res["max_abs_difference_of_the_inertia_term"] = float((out - mu[:, :, 0]).abs().max())
    assert torch.isfinite(out).all()
    return res


def centroidal(sim, n, t):
    sim.step(torch.rand(n * 18, device=DEV) * 2 - 1)   # a state off the reset pose, in motion
    state = torch.zeros(n, abi.CM_WORDS, device=DEV)
    matrix = torch.zeros(n, 6, abi.NUM_GEN, device=DEV)
    udot = torch.rand(n, abi.NUM_GEN, device=DEV) * 20 - 10
    out = torch.zeros(n, abi.NUM_GEN, device=DEV)
    M = sim.dynamics_tensor("mass_matrix")
    root = sim.refresh(abi.TENSOR_ROOT_STATE).view(n, sim.num_actors, 13)[:, 0].clone()
    qd = sim.refresh(abi.TENSOR_DOF_STATE).view(n, abi.NUM_DOFS, 2)[:, :, 1]
    u = torch.cat([root[:, 7:13], qd], dim=1).contiguous()
    g = torch.tensor(list(sim.cfg.gravity), device=DEV)
    route = {}

    def replaced():
        sim.refresh_dynamics_tensors("mass_matrix")
        B = M[:, 0:6, :]                                                    # the momentum map about the root origin
        mom = torch.bmm(B, u.unsqueeze(2))[:, :, 0]
        m = M[:, 0, 0]
        c = torch.stack([M[:, 1, 5], M[:, 2, 3], M[:, 0, 4]], dim=1) / m[:, None]   # M[0:3, 3:6] = -m skew(c)
        A = B.clone()
        A[:, 3:6, :] -= torch.cross(c[:, :, None].expand(-1, -1, abi.NUM_GEN), B[:, 0:3, :], dim=1)
        p = mom[:, 0:3]
        ang = mom[:, 3:6] - torch.cross(c, p, dim=1)
        ke = 0.5 * (u * torch.bmm(M, u.unsqueeze(2))[:, :, 0]).sum(dim=1)
        com = root[:, 0:3] + c
        pe = -m * (com * g).sum(dim=1)
        route["state"] = torch.cat([com, p / m[:, None], p, ang, m[:, None], ke[:, None], pe[:, None], torch.zeros_like(pe)[:, None]], dim=1)
        route["matrix"] = A

    res = {"centroidal_state_and_matrix": t(lambda: sim.centroidal(state, matrix)),
           "centroidal_state_only": t(lambda: sim.centroidal(state)),
           "inverse_dynamics_all_terms": t(lambda: sim.inverse_dynamics(udot, abi.ID_ALL, out)),
           "mass_matrix_refresh_plus_torch_ops": t(replaced)}
    res["ratio_to_inverse_dynamics"] = round(res["centroidal_state_and_matrix"]["median_us"] / res["inverse_dynamics_all_terms"]["median_us"], 3)
    res["ratio_to_replaced_route"] = round(res["centroidal_state_and_matrix"]["median_us"] / res["mass_matrix_refresh_plus_torch_ops"]["median_us"], 3)
    # the two routes agree
    sim.centroidal(state, matrix)
    replaced()
    torch.cuda.synchronize()
    res["max_abs_difference_state"] = float((state - route["state"]).abs().max())
    res["max_abs_difference_matrix"] = float((matrix - route["matrix"]).abs().max())
    assert torch.isfinite(state).all() and torch.isfinite(matrix).all()
    return res


def body_accelerations(sim, n, t):
    sim.step(torch.rand(n * 18, device=DEV) * 2 - 1)   # a state off the reset pose, in motion
    nb = sim.num_bodies - (1 if sim.has_ball else 0)
    udot = torch.rand(n, abi.NUM_GEN, device=DEV) * 20 - 10
    out = torch.zeros(n, nb, 6, device=DEV)
    tau = torch.zeros(n, abi.NUM_GEN, device=DEV)
    J = sim.dynamics_tensor("jacobian").view(n, nb * 6, abi.NUM_GEN)
    ju = torch.zeros(n, nb * 6, 1, device=DEV)

    def replaced():
        sim.refresh_dynamics_tensors("jacobian")
        torch.matmul(J, udot.unsqueeze(2), out=ju)

    res = {"bytes_out": out.numel() * 4,
           "body_accelerations_motion_env": t(lambda: sim.body_accelerations(udot, abi.ACC_MOTION, abi.SPACE_ENV, out)),
           "body_accelerations_all_local": t(lambda: sim.body_accelerations(udot, abi.ACC_ALL, abi.SPACE_LOCAL, out)),
           "body_accelerations_velocity_only": t(lambda: sim.body_accelerations(None, abi.ACC_VELOCITY, abi.SPACE_ENV, out)),
           "refresh_rigid_body_state": t(lambda: sim.refresh(abi.TENSOR_RIGID_BODY_STATE)),
           "inverse_dynamics_all_terms": t(lambda: sim.inverse_dynamics(udot, abi.ID_ALL, tau)),
           "jacobian_refresh_plus_matmul": t(replaced)}
    mine = res["body_accelerations_motion_env"]["median_us"]
    res["ratio_to_rigid_body_refresh"] = round(mine / res["refresh_rigid_body_state"]["median_us"], 3)
    res["ratio_to_inverse_dynamics"] = round(mine / res["inverse_dynamics_all_terms"]["median_us"], 3)
    res["ratio_to_replaced_route"] = round(mine / res["jacobian_refresh_plus_matmul"]["median_us"], 3)
    # the two routes agree on the UDOT term
    sim.body_accelerations(udot, abi.ACC_UDOT, abi.SPACE_ENV, out)
    replaced()
    torch.cuda.synchronize()
    res["max_abs_difference_of_the_udot_term"] = float((out.view(n, nb * 6) - ju[:, :, 0]).abs().max())
    assert torch.isfinite(out).all()
    return res


def generalized_forces(sim, n, t):
    sim.step(torch.rand(n * 18, device=DEV) * 2 - 1)   # a state off the reset pose
    nbe = sim.num_bodies
    nb = nbe - (1 if sim.has_ball else 0)
    F, T = torch.rand(n, nbe, 3, device=DEV) * 20 - 10, torch.rand(n, nbe, 3, device=DEV) * 2 - 1
    X = sim.refresh(abi.TENSOR_RIGID_BODY_STATE).view(n, nbe, 13)[:, :, 0:3] + (torch.rand(n, nbe, 3, device=DEV) * 0.2 - 0.1)
    X = X.contiguous()
    F1, T1 = torch.zeros_like(F), torch.zeros_like(T)
    F1[:, nb - 1], T1[:, nb - 1] = F[:, nb - 1], T[:, nb - 1]   # a foot (with cleats: its last cleat)
    out = torch.zeros(n, abi.NUM_GEN, device=DEV)
    tau = torch.zeros(n, abi.NUM_GEN, device=DEV)
    udot = torch.rand(n, abi.NUM_GEN, device=DEV) * 20 - 10
    J = sim.dynamics_tensor("jacobian").view(n, nb, 6, abi.NUM_GEN)
    W = torch.cat([F[:, :nb], T[:, :nb]], dim=2).contiguous()
    jw = torch.zeros(n, abi.NUM_GEN, device=DEV)

    def replaced():
        sim.refresh_dynamics_tensors("jacobian")
        jw.copy_(torch.einsum("ebrc,ebr->ec", J, W))

    res = {"bytes_in": 3 * F.numel() * 4, "bytes_out": out.numel() * 4,
           "generalized_forces_all_bodies": t(lambda: sim.generalized_forces(F, T, X, abi.SPACE_ENV, out=out)),
           "generalized_forces_all_bodies_local": t(lambda: sim.generalized_forces(F, T, X, abi.SPACE_LOCAL, out=out)),
           "generalized_forces_all_bodies_at_origin": t(lambda: sim.generalized_forces(F, T, None, abi.SPACE_ENV, "origin", out=out)),
           "generalized_forces_one_body": t(lambda: sim.generalized_forces(F1, T1, X, abi.SPACE_ENV, out=out)),
           "refresh_rigid_body_state": t(lambda: sim.refresh(abi.TENSOR_RIGID_BODY_STATE)),
           "inverse_dynamics_all_terms": t(lambda: sim.inverse_dynamics(udot, abi.ID_ALL, tau)),
           "jacobian_refresh_plus_einsum": t(replaced)}
    mine = res["generalized_forces_all_bodies"]["median_us"]
    res["ratio_to_rigid_body_refresh"] = round(mine / res["refresh_rigid_body_state"]["median_us"], 3)
    res["ratio_to_inverse_dynamics"] = round(mine / res["inverse_dynamics_all_terms"]["median_us"], 3)
    res["ratio_to_replaced_route"] = round(res["generalized_forces_all_bodies_at_origin"]["median_us"] / res["jacobian_refresh_plus_einsum"]["median_us"], 3)
    # the two routes agree
    sim.generalized_forces(F, T, None, abi.SPACE_ENV, "origin", out=out)
    replaced()
    torch.cuda.synchronize()
    res["max_abs_difference_of_the_two_routes"] = float((out - jw).abs().max())
    assert torch.isfinite(out).all()
    return res


def limb_ik(sim, n, t):
    sim.step(torch.rand(n * 18, device=DEV) * 2 - 1)   # a state off the reset pose
    nbe = sim.num_bodies
    nb = nbe - (1 if sim.has_ball else 0)
    names = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "bez_isaacgym_amd", "model", "bez_model.json")))
    names = (names["cleats"] if int(sim.cfg.flags) & abi.FLAG_CLEATS else names)["body_names"]
    ends = [names.index(b) for b in abi.IK_END_BODIES]
    rb = sim.refresh(abi.TENSOR_RIGID_BODY_STATE).view(n, nbe, 13)
    T = rb[:, ends, 0:7].clone()
    T[:, :, 0:3] += torch.rand(n, 5, 3, device=DEV) * 0.06 - 0.03        # 3 cm and about 0.1 rad off the current poses
    T[:, :, 3:7] += torch.rand(n, 5, 4, device=DEV) * 0.1 - 0.05
    T = T.contiguous()
    w, lam = [[1.0, 0.25]] * abi.IK_CHAINS, 0.05
    q, err = torch.zeros(n, abi.NUM_DOFS, device=DEV), torch.zeros(n, abi.IK_CHAINS, 6, device=DEV)
    J = sim.dynamics_tensor("jacobian").view(n, nb, 6, abi.NUM_GEN)
    q0 = sim.refresh(abi.TENSOR_DOF_STATE).view(n, abi.NUM_DOFS, 2)[:, :, 0].clone()
    W6 = torch.tensor([1.0, 1.0, 1.0, 0.25, 0.25, 0.25], device=DEV)
    route = {}

    def replaced():   # Isaac's pattern: refresh the body states and the Jacobian tensor, slice a limb's columns, solve in torch (world axes)
        sim.refresh_dynamics_tensors("jacobian")
        cur = sim.refresh(abi.TENSOR_RIGID_BODY_STATE).view(n, nbe, 13)[:, ends, 0:7]
        td = T[:, :, 3:7] / T[:, :, 3:7].norm(dim=2, keepdim=True)
        dv, dw, cv, cw = td[:, :, 0:3], td[:, :, 3:4], -cur[:, :, 3:6], cur[:, :, 6:7]          # q_des * conj(q)
        ev = dw * cv + cw * dv + torch.cross(dv, cv, dim=2)
        ew = dw * cw - (dv * cv).sum(dim=2, keepdim=True)
        e = torch.cat([T[:, :, 0:3] - cur[:, :, 0:3], 2.0 * torch.where(ew < 0, -ev, ev)], dim=2)
        dq = torch.zeros(n, abi.NUM_DOFS, device=DEV)
        for c, (d0, d1) in enumerate(abi.IK_CHAIN_DOFS):
            Jc = J[:, ends[c], :, 6 + d0:6 + d1]
            JW = Jc.transpose(1, 2) * W6
            N = JW @ Jc + lam * lam * torch.eye(d1 - d0, device=DEV)
            dq[:, d0:d1] = torch.linalg.solve(N, (JW @ e[:, c, :, None]))[:, :, 0]
        route["q"] = q0 + dq

    big = torch.full((n, abi.NUM_DOFS), 100.0, device=DEV)
    res = {"bytes_in": T.numel() * 4, "bytes_out": (q.numel() + err.numel()) * 4,
           "limb_ik_iters_1": t(lambda: sim.limb_ik(T, w, None, lam, 0.0, 1, "env", q, err)),
           "limb_ik_iters_8": t(lambda: sim.limb_ik(T, w, None, lam, 0.0, 8, "env", q, err)),
           "limb_ik_iters_0_pose_error": t(lambda: sim.limb_ik(T, w, None, lam, 0.0, 0, "env", q, err)),
           "limb_ik_iters_8_legs_only": t(lambda: sim.limb_ik(T, [[0.0, 0.0], [0.0, 0.0], [1.0, 0.25], [0.0, 0.0], [1.0, 0.25]], None, lam, 0.2, 8, "env", q, err)),
           "refresh_rigid_body_state": t(lambda: sim.refresh(abi.TENSOR_RIGID_BODY_STATE)),
           "jacobian_refresh_plus_torch_solve_one_iteration": t(replaced)}
    rbs = res["refresh_rigid_body_state"]["median_us"]
    res["ratio_to_rigid_body_refresh"] = {"iters_1": round(res["limb_ik_iters_1"]["median_us"] / rbs, 3), "iters_8": round(res["limb_ik_iters_8"]["median_us"] / rbs, 3)}
    one = res["jacobian_refresh_plus_torch_solve_one_iteration"]["median_us"]
    res["ratio_to_replaced_route"] = {"iters_1": round(res["limb_ik_iters_1"]["median_us"] / one, 4), "iters_8_to_one_iteration_of_it": round(res["limb_ik_iters_8"]["median_us"] / one, 4)}
    # the two routes agree on one unclamped step
    sim.set_env_params(abi.PARAM_DOF_LOWER, (-big).reshape(-1))
    sim.set_env_params(abi.PARAM_DOF_UPPER, big.reshape(-1))
    sim.limb_ik(T, w, None, lam, 0.0, 1, "env", q, err)
    replaced()
    torch.cuda.synchronize()
    res["max_abs_difference_of_the_two_routes_rad"] = float((q - route["q"]).abs().max())
    assert torch.isfinite(q).all() and torch.isfinite(err).all()
    return res


def proximity(sim, n, t):
    sim.step(torch.rand(n * 18, device=DEV) * 2 - 1)   # a state off the reset pose
    nbe = sim.num_bodies
    assert sim.has_ball, "the replaced route reads the ball's body row"
    m = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "bez_isaacgym_amd", "model", "bez_model.json")))
    cl = bool(int(sim.cfg.flags) & abi.FLAG_CLEATS)
    link_body = [L["body"] for L in (m["cleats"] if cl else m)["links"]]
    dev = lambda rows, key: torch.tensor([r[key] for r in rows], device=DEV, dtype=torch.float32)
    body_of = lambda rows: torch.tensor([link_body[r["link"]] for r in rows], device=DEV)
    pts = (m["cleats"] if cl else m)["ground_points"]
    pt_body, pt_p = body_of(pts), dev(pts, "p")
    box_body, box_c, box_h = body_of(m["boxes"]), dev(m["boxes"], "center"), dev(m["boxes"], "half")
    cap_body, cap_p0, cap_p1, cap_r = body_of(m["capsules"]), dev(m["capsules"], "p0"), dev(m["capsules"], "p1"), dev(m["capsules"], "r")
    ia, ib = (torch.tensor([p[k] for p in m["capsule_pairs"]], device=DEV) for k in (0, 1))
    R = float(m["ball"]["radius"])
    ground, ball, pairs = (torch.zeros(n, r, w, device=DEV) for r, w in ((abi.PROX_GROUND_ROWS, 3), (abi.PROX_BOXES, 8), (abi.PROX_PAIRS, 8)))
    route = {}

    def rot(q):   # (..., 4) xyzw -> (..., 3, 3)
        x, y, z, w = q.unbind(-1)
        return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w), 2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                            2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], dim=-1).view(q.shape[:-1] + (3, 3))

    def replaced():
        rb = sim.refresh(abi.TENSOR_RIGID_BODY_STATE).view(n, nbe, 13)
        pos, E = rb[:, :, 0:3], rot(rb[:, :, 3:7])
        centre = pos[:, nbe - 1]
        low = centre.clone()
        low[:, 2] -= R
        g = torch.cat([pos[:, pt_body] + (E[:, pt_body] @ pt_p[None, :, :, None])[..., 0], low[:, None]], dim=1)
        Eb = E[:, box_body]
        ql = (Eb.transpose(2, 3) @ (centre[:, None] - pos[:, box_body])[..., None])[..., 0] - box_c
        cp = torch.minimum(torch.maximum(ql, -box_h), box_h)
        inside = (cp == ql).all(dim=2)
        dlt = ql - cp
        dist = dlt.norm(dim=2)
        face = box_h - ql.abs()
        md, ax = face.min(dim=2)
        sgn = torch.where(ql.gather(2, ax[..., None])[..., 0] >= 0, 1.0, -1.0)
        n_in = torch.zeros_like(ql).scatter(2, ax[..., None], sgn[..., None])
        cp_in = cp.scatter(2, ax[..., None], (sgn * box_h.expand_as(ql).gather(2, ax[..., None])[..., 0])[..., None])
        gap = torch.where(inside, -(R + md), dist - R)
        nl = torch.where(inside[..., None], n_in, dlt / dist[..., None])
        cpl = torch.where(inside[..., None], cp_in, cp) + box_c
        b = torch.cat([gap[..., None], (Eb @ nl[..., None])[..., 0], pos[:, box_body] + (Eb @ cpl[..., None])[..., 0], torch.zeros_like(gap)[..., None]], dim=2)
        Ec, pc = E[:, cap_body], pos[:, cap_body]
        c0, c1 = pc + (Ec @ cap_p0[None, :, :, None])[..., 0], pc + (Ec @ cap_p1[None, :, :, None])[..., 0]
        p1, p2 = c0[:, ia], c0[:, ib]
        d1, d2 = c1[:, ia] - p1, c1[:, ib] - p2
        r = p1 - p2
        a, e, f, c, bb = (d1 * d1).sum(2), (d2 * d2).sum(2), (d2 * r).sum(2), (d1 * r).sum(2), (d1 * d2).sum(2)
        den = a * e - bb * bb
        s = torch.where(den > 1e-12, ((bb * f - c * e) / den).clamp(0, 1), torch.zeros_like(den))
        tt = (bb * s + f) / e
        tc = tt.clamp(0, 1)
        s = torch.where(tt != tc, ((bb * tc - c) / a).clamp(0, 1), s)
        ca, cb = p1 + d1 * s[..., None], p2 + d2 * tc[..., None]
        dl = ca - cb
        dd = dl.norm(dim=2)
        rs, rbr = cap_r[ia] + cap_r[ib], cap_r[ib]
        pg = dd - rs
        pn = dl / dd[..., None]
        p = torch.cat([pg[..., None], pn, cb + pn * (rbr + 0.5 * pg)[..., None], torch.zeros_like(pg)[..., None]], dim=2)
        route["ground"], route["ball"], route["pairs"] = g, b, p

    res = {"bytes_out": (ground.numel() + ball.numel() + pairs.numel()) * 4,
           "proximity_all": t(lambda: sim.proximity(ground, ball, pairs)),
           "proximity_ground_only": t(lambda: sim.proximity(ground=ground, want=())),
           "proximity_ball_only": t(lambda: sim.proximity(ball=ball, want=())),
           "proximity_pairs_only": t(lambda: sim.proximity(pairs=pairs, want=())),
           "refresh_rigid_body_state": t(lambda: sim.refresh(abi.TENSOR_RIGID_BODY_STATE)),
           "rigid_body_refresh_plus_torch_ops": t(replaced)}
    mine = res["proximity_all"]["median_us"]
    res["ratio_to_rigid_body_refresh"] = round(mine / res["refresh_rigid_body_state"]["median_us"], 3)
    res["ratio_to_replaced_route"] = round(mine / res["rigid_body_refresh_plus_torch_ops"]["median_us"], 4)
    # the two routes agree (the replaced route works on body rows that carry the root position: its points are rounded at that size)
    sim.proximity(ground, ball, pairs)
    replaced()
    torch.cuda.synchronize()
    res["max_abs_difference_ground_m"] = float((ground - route["ground"]).abs().max())
    res["max_abs_difference_ball_gap_m"] = float((ball[:, :, 0] - route["ball"][:, :, 0]).abs().max())
    res["max_abs_difference_pair_gap_m"] = float((pairs[:, :, 0] - route["pairs"][:, :, 0]).abs().max())
    assert torch.isfinite(ground).all() and torch.isfinite(ball).all() and torch.isfinite(pairs).all()
    return res


def forward_dynamics(sim, n, t):
    sim.step(torch.rand(n * 18, device=DEV) * 2 - 1)   # a state off the reset pose, in motion
    bias = abi.ID_VELOCITY | abi.ID_GRAVITY
    force = torch.rand(n, abi.NUM_GEN, device=DEV) - 0.5
    out = torch.zeros(n, abi.NUM_GEN, device=DEV)
    h = torch.zeros(n, abi.NUM_GEN, device=DEV)
    udot = torch.zeros(n, abi.NUM_GEN, device=DEV)
    M = sim.dynamics_tensor("mass_matrix")
    route = {}

    def replaced():
        sim.refresh_dynamics_tensors("mass_matrix")
        sim.inverse_dynamics(None, bias, h)
        route["udot"] = torch.linalg.solve(M, (force - h).unsqueeze(2))[:, :, 0]

    res = {"forward_dynamics_floating": t(lambda: sim.forward_dynamics(force, bias, False, out)),
           "forward_dynamics_fixed_base": t(lambda: sim.forward_dynamics(force, bias, True, out)),
           "forward_dynamics_mass_solve": t(lambda: sim.forward_dynamics(force, 0, False, out)),
           "inverse_dynamics_all_terms": t(lambda: sim.inverse_dynamics(udot, abi.ID_ALL, h)),
           "mass_matrix_refresh": t(lambda: sim.refresh_dynamics_tensors("mass_matrix")),
           "mass_matrix_refresh_plus_bias_plus_linalg_solve": t(replaced)}
    mine = res["forward_dynamics_floating"]["median_us"]
    res["ratio_to_inverse_dynamics"] = round(mine / res["inverse_dynamics_all_terms"]["median_us"], 3)
    res["ratio_to_replaced_route"] = round(mine / res["mass_matrix_refresh_plus_bias_plus_linalg_solve"]["median_us"], 4)
    # the two routes agree
    sim.forward_dynamics(force, bias, False, out)
    replaced()
    torch.cuda.synchronize()
    res["max_abs_difference_of_udot"] = float((out - route["udot"]).abs().max())
    res["max_abs_udot"] = float(out.abs().max())
    assert torch.isfinite(out).all()
    return res


def operational_space(sim, n, t):
    sim.step(torch.rand(n * 18, device=DEV) * 2 - 1)   # a state off the reset pose, in motion
    model = json.load(open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bez_isaacgym_amd", "model", "bez_model.json")))
    ends = torch.tensor([model["body_names"].index(b) for b in abi.IK_END_BODIES], device=DEV)
    offsets = [[0, 0, .03], [0, 0, -.05], [.02, 0, -.01], [0, 0, -.05], [.02, 0, -.01]]
    off = torch.tensor(offsets, device=DEV, dtype=torch.float32)
    nb = sim.num_bodies - (1 if sim.has_ball else 0)
    nch, nf, ng = abi.IK_CHAINS, 6 * abi.IK_CHAINS, abi.NUM_GEN
    outs = [torch.zeros(s, device=DEV) for s in ((n, nch, 6, ng), (n, nch, 6, ng), (n, nf, nf), (n, nch, 6, 6))]
    Jt, M = sim.dynamics_tensor("jacobian"), sim.dynamics_tensor("mass_matrix")
    force, udot = torch.rand(n, ng, device=DEV) - 0.5, torch.zeros(n, ng, device=DEV)
    route = {}

    def replaced(with_lambda):
        def run():
            rb = sim.refresh(abi.TENSOR_RIGID_BODY_STATE).view(n, sim.num_bodies, 13)
            sim.refresh_dynamics_tensors(["jacobian", "mass_matrix"])
            q = rb[:, ends, 3:7]
            qv, qw = q[..., 0:3], q[..., 3:4]
            o = off.unsqueeze(0).expand(n, nch, 3)
            d = o + 2.0 * torch.cross(qv, torch.cross(qv, o, dim=-1) + qw * o, dim=-1)        # the offsets in world axes
            J = Jt.view(n, nb, 6, ng)[:, ends].clone()
            J[:, :, 0:3] += torch.cross(J[:, :, 3:6], d.unsqueeze(3).expand(n, nch, 3, ng), dim=2)   # v + w x d, column by column
            JE = J.view(n, nf, ng)
            T = torch.linalg.solve(M, JE.transpose(1, 2))
            route["jac"], route["jminv"], route["w"] = J, T.transpose(1, 2), torch.bmm(JE, T)
            if with_lambda:
                route["lambda"] = torch.linalg.inv(torch.stack([route["w"][:, 6 * c:6 * c + 6, 6 * c:6 * c + 6] for c in range(nch)], dim=1))
        return run

    res = {"operational_space_all_outputs": t(lambda: sim.operational_space(offsets, False, *outs)),
           "operational_space_w_alone": t(lambda: sim.operational_space(offsets, False, w=outs[2], want=())),
           "operational_space_fixed_base": t(lambda: sim.operational_space(offsets, True, outs[0], outs[1], outs[2], want=())),
           "forward_dynamics_mass_solve": t(lambda: sim.forward_dynamics(force, 0, False, udot)),
           "refreshes_slice_shift_linalg_solve_bmm": t(replaced(False)),
           "refreshes_slice_shift_linalg_solve_bmm_plus_linalg_inv": t(replaced(True))}
    mine = res["operational_space_all_outputs"]["median_us"]
    res["ratio_to_forward_dynamics_mass_solve"] = round(mine / res["forward_dynamics_mass_solve"]["median_us"], 3)
    res["ratio_to_replaced_route"] = round(mine / res["refreshes_slice_shift_linalg_solve_bmm"]["median_us"], 4)
    res["ratio_to_replaced_route_with_lambda"] = round(mine / res["refreshes_slice_shift_linalg_solve_bmm_plus_linalg_inv"]["median_us"], 4)
    # the two routes agree
    sim.operational_space(offsets, False, *outs)
    replaced(True)()
    torch.cuda.synchronize()
    for k, mine_t in zip(("jac", "jminv", "w", "lambda"), outs):
        res["max_abs_difference_of_" + k] = float((mine_t - route[k].reshape(mine_t.shape)).abs().max())
        res["max_abs_" + k] = float(mine_t.abs().max())
        assert torch.isfinite(mine_t).all()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("call", choices=["tensors", "inverse_dynamics", "centroidal", "body_accelerations", "generalized_forces", "limb_ik", "proximity", "forward_dynamics", "operational_space"])
    ap.add_argument("--num-envs", type=int, default=4096)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--cleats", action="store_true")
    args = ap.parse_args()
    cfg = abi.default_config(args.num_envs)
    if args.cleats:
        cfg.flags |= abi.FLAG_CLEATS
    sim = BezSim(cfg, 0)
    res = {"num_envs": args.num_envs, "launches": args.launches, "warmup": args.warmup, "device": torch.cuda.get_device_name(0)}
    res.update(globals()[args.call](sim, args.num_envs, lambda fn: timed(fn, args.launches, args.warmup)))
    sim.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
