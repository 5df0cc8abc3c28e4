"""Times bez_sim_refresh_dynamics_tensors (the Jacobian, the mass matrix, both) at num_envs = 4096 beside a plain device fill of the
same bytes in the same run -- the kernel is store-bound by construction, so the fill is its yardstick.

Each figure is the median over --launches (>= 200) single launches, each between its own pair of events on one stream, after --warmup
launches; the fill is hipMemsetAsync over the very buffer the refresh writes, timed the same way.  Nothing flushes the caches between
launches, for the refresh and the fill alike.  Prints one JSON line.

  python tools/dynamics_bench.py [--num-envs 4096] [--launches 200] [--warmup 20] [--cleats]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--num-envs", type=int, default=4096)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--cleats", action="store_true")
    args = ap.parse_args()
    cfg = abi.default_config(args.num_envs)
    if args.cleats:
        cfg.flags |= abi.FLAG_CLEATS
    sim = BezSim(cfg, 0)
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemsetAsync.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p]
    hip.hipMemsetAsync.restype = C.c_int
    act = torch.zeros(args.num_envs * 18, device="cuda:0")
    sim.step(act)   # a state off the reset pose
    J, M = sim.dynamics_tensor("jacobian"), sim.dynamics_tensor("mass_matrix")
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def fill(*tensors):
        def run():
            for t in tensors:
                assert hip.hipMemsetAsync(C.c_void_p(t.data_ptr()), 0, t.numel() * 4, stream()) == 0
        return run

    out = {"num_envs": args.num_envs, "launches": args.launches, "warmup": args.warmup, "device": torch.cuda.get_device_name(0),
           "bytes": {"jacobian": J.numel() * 4, "mass_matrix": M.numel() * 4}}
    for name, which, tensors in (("jacobian", ["jacobian"], (J,)), ("mass_matrix", ["mass_matrix"], (M,)), ("both", ["jacobian", "mass_matrix"], (J, M))):
        r = timed(lambda: sim.refresh_dynamics_tensors(which), args.launches, args.warmup)
        f = timed(fill(*tensors), args.launches, args.warmup)
        nbytes = sum(t.numel() * 4 for t in tensors)
        out[name] = {"refresh": r, "fill": f, "ratio": round(r["median_us"] / f["median_us"], 3),
                     "refresh_GBps": round(nbytes / r["median_us"] / 1e3, 1), "fill_GBps": round(nbytes / f["median_us"] / 1e3, 1)}
    sim.refresh_dynamics_tensors()
    torch.cuda.synchronize()
    assert torch.isfinite(J).all() and torch.isfinite(M).all()
    sim.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
