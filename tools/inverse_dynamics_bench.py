"""Times bez_sim_inverse_dynamics (all terms) at num_envs = 4096 beside, in the same run, refresh_rigid_body_state -- the same per-lane
forward kinematics -- and the route the call replaces: a mass-matrix refresh followed by torch.bmm(M, udot).

Each figure is the median over --launches (>= 200) single launches, each between its own pair of events on one stream, after --warmup
launches (tools/dynamics_bench.py's method).  Nothing flushes the caches between launches.  Prints one JSON line.

  python tools/inverse_dynamics_bench.py [--num-envs 4096] [--launches 200] [--warmup 20] [--cleats]
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
    sim.step(torch.zeros(n * 18, device="cuda:0"))   # a state off the reset pose
    udot = torch.rand(n, abi.NUM_GEN, device="cuda:0") * 20 - 10
    out = torch.zeros(n, abi.NUM_GEN, device="cuda:0")
    M = sim.dynamics_tensor("mass_matrix")
    mu = torch.zeros(n, abi.NUM_GEN, 1, device="cuda:0")

    def replaced():
        sim.refresh_dynamics_tensors("mass_matrix")
        torch.bmm(M, udot.unsqueeze(2), out=mu)

    res = {"num_envs": n, "launches": args.launches, "warmup": args.warmup, "device": torch.cuda.get_device_name(0),
           "inverse_dynamics_all_terms": timed(lambda: sim.inverse_dynamics(udot, abi.ID_ALL, out), args.launches, args.warmup),
           "inverse_dynamics_gravity_only": timed(lambda: sim.inverse_dynamics(None, abi.ID_GRAVITY, out), args.launches, args.warmup),
           "refresh_rigid_body_state": timed(lambda: sim.refresh(abi.TENSOR_RIGID_BODY_STATE), args.launches, args.warmup),
           "mass_matrix_refresh_plus_bmm": timed(replaced, args.launches, args.warmup)}
    res["ratio_to_rigid_body_refresh"] = round(res["inverse_dynamics_all_terms"]["median_us"] / res["refresh_rigid_body_state"]["median_us"], 3)
    res["ratio_to_replaced_route"] = round(res["inverse_dynamics_all_terms"]["median_us"] / res["mass_matrix_refresh_plus_bmm"]["median_us"], 3)
    # the two routes agree on the inertia term
    sim.inverse_dynamics(udot, abi.ID_INERTIA, out)
    replaced()
    torch.cuda.synchronize()
    res["max_abs_difference_of_the_inertia_term"] = float((out - mu[:, :, 0]).abs().max())
    assert torch.isfinite(out).all()
    sim.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
