"""Times bez_sim_centroidal at num_envs = 4096 (both outputs; the state alone) beside, in the same run, bez_sim_inverse_dynamics with all
terms -- the neighbour of the same shape -- and the route the call replaces: a mass-matrix refresh followed by the torch ops that rebuild
the 16 + 144 numbers per env from M and u (rows 0:6 of M times u, the centre of mass un-skewed from M[0:3, 3:6], the moment shifted to
it, 1/2 u^T M u).  The replaced route is handed u and the root positions ready-made: refreshing them is not counted against it.

Each figure is the median over --launches (>= 200) single launches, each between its own pair of events on one stream, after --warmup
launches (tools/dynamics_bench.py's method).  Nothing flushes the caches between launches.  Prints one JSON line.

  python tools/centroidal_bench.py [--num-envs 4096] [--launches 200] [--warmup 20] [--cleats]
  python tools/centroidal_bench.py > profiles/centroidal_bench.json      (the committed record)
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bez_isaacgym_amd import abi  # noqa: E402
from bez_isaacgym_amd.sim import BezSim  # noqa: E402
from tools.dynamics_bench import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--num-envs", type=int, default=4096)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--cleats", action="store_true")
    args = ap.parse_args()
    n = args.num_envs
    cfg = abi.default_config(n)
    if args.cleats:
        cfg.flags |= abi.FLAG_CLEATS
    sim = BezSim(cfg, 0)
    sim.step(torch.rand(n * 18, device="cuda:0") * 2 - 1)   # a state off the reset pose, in motion
    state = torch.zeros(n, abi.CM_WORDS, device="cuda:0")
    matrix = torch.zeros(n, 6, abi.NUM_GEN, device="cuda:0")
    udot = torch.rand(n, abi.NUM_GEN, device="cuda:0") * 20 - 10
    out = torch.zeros(n, abi.NUM_GEN, device="cuda:0")
    M = sim.dynamics_tensor("mass_matrix")
    root = sim.refresh(abi.TENSOR_ROOT_STATE).view(n, sim.num_actors, 13)[:, 0].clone()
    qd = sim.refresh(abi.TENSOR_DOF_STATE).view(n, abi.NUM_DOFS, 2)[:, :, 1]
    u = torch.cat([root[:, 7:13], qd], dim=1).contiguous()
    g = torch.tensor(list(cfg.gravity), device="cuda:0")
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

    res = {"num_envs": n, "launches": args.launches, "warmup": args.warmup, "device": torch.cuda.get_device_name(0),
           "centroidal_state_and_matrix": timed(lambda: sim.centroidal(state, matrix), args.launches, args.warmup),
           "centroidal_state_only": timed(lambda: sim.centroidal(state), args.launches, args.warmup),
           "inverse_dynamics_all_terms": timed(lambda: sim.inverse_dynamics(udot, abi.ID_ALL, out), args.launches, args.warmup),
           "mass_matrix_refresh_plus_torch_ops": timed(replaced, args.launches, args.warmup)}
    res["ratio_to_inverse_dynamics"] = round(res["centroidal_state_and_matrix"]["median_us"] / res["inverse_dynamics_all_terms"]["median_us"], 3)
    res["ratio_to_replaced_route"] = round(res["centroidal_state_and_matrix"]["median_us"] / res["mass_matrix_refresh_plus_torch_ops"]["median_us"], 3)
    # the two routes agree
    sim.centroidal(state, matrix)
    replaced()
    torch.cuda.synchronize()
    res["max_abs_difference_state"] = float((state - route["state"]).abs().max())
    res["max_abs_difference_matrix"] = float((matrix - route["matrix"]).abs().max())
    assert torch.isfinite(state).all() and torch.isfinite(matrix).all()
    sim.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
