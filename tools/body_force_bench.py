"""Cost of the external-force path (bez_sim_apply_body_forces) on the fused step, in one process: the default kernel (BEZ_SIM_KERNEL
unset: the lane-group form up to 16 x CUs envs) and the one-lane 8-role-wave kernel (ws8), each in three cases --
  default   a sim that never applies a force (the kernels it always ran)
  ext_idle  a sim switched to the force-carrying kernels by one apply call, with nothing pending afterwards
  ext_push  a force on every body of every env before every step (the apply call's prepare kernel included)
Rounds alternate over the six sims; each round times `steps` steps with device events on the current stream.  Prints one JSON line.
usage: python tools/body_force_bench.py [--envs 4096] [--steps 200] [--rounds 7]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bez_isaacgym_amd import abi  # noqa: E402
from bez_isaacgym_amd.sim import BezSim  # noqa: E402


def make(kernel, n):
    if kernel == "default":
        os.environ.pop("BEZ_SIM_KERNEL", None)
    else:
        os.environ["BEZ_SIM_KERNEL"] = kernel
    return BezSim(abi.default_config(n, seed=1), 0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    n = a.envs
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(0)
    acts = torch.rand((a.steps, n, 18), device=dev, generator=gen) * 2 - 1
    sims = {}
    for kernel in ("default", "ws8"):
        for case in ("default", "ext_idle", "ext_push"):
            s = make(kernel, n)
            if case != "default":
                s.apply_body_forces(forces=torch.zeros((n, s.num_bodies, 3), device=dev))
            sims[(kernel, case)] = s
    os.environ.pop("BEZ_SIM_KERNEL", None)
    push = (torch.rand((n, 22, 3), device=dev, generator=gen) * 2 - 1) * 5.0
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def run(key, steps):
        s = sims[key]
        for t in range(steps):
            if key[1] == "ext_push":
                s.apply_body_forces(forces=push)
            s.step(acts[t].reshape(-1))

    for key in sims:   # warm-up
        run(key, 20)
    torch.cuda.synchronize()
    times = {key: [] for key in sims}
    for _ in range(a.rounds):
        for key in sims:
            ev0.record()
            run(key, a.steps)
            ev1.record()
            ev1.synchronize()
            times[key].append(ev0.elapsed_time(ev1) * 1e3 / a.steps)
    out = {"envs": n, "steps": a.steps, "rounds": a.rounds, "us_per_step": {}}
    for (kernel, case), v in times.items():
        out["us_per_step"]["%s/%s" % (kernel, case)] = {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}
    for kernel in ("default", "ws8"):
        base = out["us_per_step"]["%s/default" % kernel]["median"]
        for case in ("ext_idle", "ext_push"):
            out["us_per_step"]["%s/%s" % (kernel, case)]["vs_default"] = out["us_per_step"]["%s/%s" % (kernel, case)]["median"] / base - 1.0
    print(json.dumps(out))


if __name__ == "__main__":
    main()
