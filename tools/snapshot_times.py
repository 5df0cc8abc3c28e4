"""Launch times of the env-snapshot calls on the GPU: save and restore at M = N rows on bez_kick with every parameter
row allocated, for the identity and for a permutation, against the floor they are judged by -- one plain device-to-device copy of as
many bytes as the snapshot's columns hold.

    python tools/snapshot_times.py [--rows 4096] [--calls 1000] [--windows 7]

Each number is device-event time over a window of `calls` back-to-back calls on one stream, divided by `calls`, after a warm-up of the
same shape; the median of `windows` windows and their spread (max - min) are reported.  The legs alternate window by window, so all
see the same drift of the machine.  The *_one_wg_per_tile legs are the same calls on a snapshot created under BEZ_SNAPSHOT_GRID_Y=1: one
workgroup per tile of 64 entries walks all chunks of columns, the tiling of the query-state fill, against one workgroup per tile and
chunk.  A restore here is two launches: the copy kernel and the rebuild of the packed gains and limits.  One JSON line."""
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
    ap.add_argument("--calls", type=int, default=1000)
    ap.add_argument("--windows", type=int, default=7)
    args = ap.parse_args()
    m = args.rows
    sim = BezSim(abi.default_config(m, seed=3), 0)
    rng = np.random.default_rng(0)
    for p in range(len(abi.PARAM_WIDTH)):     # every parameter row allocated: all seven sections move
        rows = sim.get_env_params(p)
        sim.set_env_params(p, rows * torch.as_tensor(rng.uniform(0.99, 1.01, tuple(rows.shape)), dtype=torch.float32, device=sim.device))
    act = torch.as_tensor(rng.uniform(-1, 1, (m, 18)), dtype=torch.float32, device=sim.device)
    for _ in range(20):
        sim.step(act)
    ids = torch.as_tensor(rng.permutation(m).astype(np.int32), device=sim.device)
    snap = sim.snapshot(m)
    snap.save()
    os.environ["BEZ_SNAPSHOT_GRID_Y"] = "1"
    flat = sim.snapshot(m)
    del os.environ["BEZ_SNAPSHOT_GRID_Y"]
    flat.save()
    words = snap._blob_words() - abi.SNAPSHOT_HEADER_WORDS
    src, dst = torch.zeros(words, dtype=torch.int32, device=sim.device), torch.zeros(words, dtype=torch.int32, device=sim.device)
    legs = {
        "save": lambda: snap.save(),
        "save_env_ids": lambda: snap.save(ids),
        "restore": lambda: snap.restore(),
        "restore_globals": lambda: snap.restore(globals_=True),
        "restore_ids": lambda: snap.restore(env_ids=ids, row_ids=ids),
        "save_one_wg_per_tile": lambda: flat.save(),
        "restore_one_wg_per_tile": lambda: flat.restore(),
        "memcpy_d2d": lambda: dst.copy_(src, non_blocking=True),
    }
    for fn in legs.values():           # warm-up: code objects
        for _ in range(min(50, max(1, args.calls))):
            fn()
    snap.save()                        # (identity rows again: the timed restores put back what the envs hold)
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(args.windows):      # the legs alternate window by window
        for k, fn in legs.items():
            times[k].append(window_us(fn, args.calls))
    out = {"rows": m, "bytes": words * 4, "bytes_per_row": words * 4 // m, "calls_per_window": args.calls, "windows": args.windows,
           "unit": "us per call, device events", "device": torch.cuda.get_device_name(0)}
    for k, v in times.items():
        out[k] = {"median": round(float(np.median(v)), 3), "spread": round(float(max(v) - min(v)), 3)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
