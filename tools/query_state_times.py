"""Launch times of the query-state calls on the GPU: set and capture with and without env ids, and inverse_dynamics and
operational_space on a query state against the same calls on the live state, at M = N rows.

    python tools/query_state_times.py [--rows 4096] [--calls 2000] [--windows 7]

Each number is device-event time over a window of `calls` back-to-back launches on one stream, divided by `calls`, after a warm-up of the
same shape; the median of `windows` windows and their spread (max - min) are reported.  The live and the query-state variant of a call
alternate window by window, so both see the same drift of the machine.  One JSON line."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bez_isaacgym_amd import abi  # noqa: E402
from bez_isaacgym_amd.sim import BezSim  # noqa: E402


def window_us(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1000.0 / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--calls", type=int, default=2000)
    ap.add_argument("--windows", type=int, default=7)
    args = ap.parse_args()
    m = args.rows
    sim = BezSim(abi.default_config(m, seed=3), 0)
    rng = np.random.default_rng(0)
    for p in abi.QUERY_PARAMS:     # per-env rows, so that a set with ids gathers all four
        rows = sim.get_env_params(p)
        sim.set_env_params(p, rows * torch.as_tensor(rng.uniform(0.9, 1.1, tuple(rows.shape)), dtype=torch.float32, device=sim.device))
    act = torch.as_tensor(rng.uniform(-1, 1, (m, 18)), dtype=torch.float32, device=sim.device)
    for _ in range(20):
        sim.step(act)
    root = sim.refresh(abi.TENSOR_ROOT_STATE).view(m, 2, 13)
    robot, ball = root[:, 0].contiguous(), root[:, 1].contiguous()
    dof = sim.refresh(abi.TENSOR_DOF_STATE).view(m, 18, 2).clone()
    ids = torch.as_tensor(rng.permutation(m).astype(np.int32), device=sim.device)
    qs = sim.query_state(m)
    qs.capture()
    udot = torch.as_tensor(rng.uniform(-10, 10, (m, 24)), dtype=torch.float32, device=sim.device)
    legs = {
        "set": lambda: qs.set(robot, dof, ball),
        "set_env_ids": lambda: qs.set(robot, dof, ball, ids),
        "capture": lambda: qs.capture(),
        "capture_env_ids": lambda: qs.capture(ids),
        "inverse_dynamics_live": lambda: sim.inverse_dynamics(udot),
        "inverse_dynamics_query_state": lambda: qs.inverse_dynamics(udot),
        "operational_space_live": lambda: sim.operational_space(),
        "operational_space_query_state": lambda: qs.operational_space(),
    }
    for fn in legs.values():           # warm-up: code objects, result buffers
        for _ in range(50):
            fn()
    qs.capture()                       # (the timed queries read the live state's rows, as the live calls do)
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(args.windows):      # the legs alternate window by window
        for k, fn in legs.items():
            times[k].append(window_us(fn, args.calls))
    out = {"rows": m, "calls_per_window": args.calls, "windows": args.windows, "unit": "us per call, device events",
           "device": torch.cuda.get_device_name(0)}
    for k, v in times.items():
        out[k] = {"median": round(float(np.median(v)), 3), "spread": round(float(max(v) - min(v)), 3)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
