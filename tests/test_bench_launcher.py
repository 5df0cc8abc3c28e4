"""`python bench.py --gpus N` must start N ranks itself: launcher plumbing on the CPU with gloo and a
stub step -- rendezvous on 127.0.0.1, RANK / LOCAL_RANK / WORLD_SIZE per child, rank 0's ONE JSON line relayed, n_gpus = N."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, env=None):
    e = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        e.pop(k, None)
    e.update(env or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=e, capture_output=True, text=True, timeout=300)


def test_bench_gpus_2_launches_two_ranks():
    r = _run(["--gpus", "2", "--steps", "5", "--warmup", "1", "--stub-cpu"])
    assert r.returncode == 0, r.stderr
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout  # only rank 0 prints
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["config"]["parallelism"] == "env-sharded x2" and d["steps"] == 5 and d["warmup"] == 1
    assert d["collective"] == {"backend": "gloo", "world_size": 2, "rank_sum_check": True} and d["cpu_baseline"] == "N=1 only"


def test_a_dying_rank_takes_the_job_down():
    """the launcher used to wait for its children one after the other -- rank 1 dying left rank 0 in the
    rendezvous for ever.  Now every child is polled, the survivor is terminated and the failing code is returned."""
    import time
    t0 = time.time()
    r = _run(["--gpus", "2", "--steps", "5", "--warmup", "1", "--stub-cpu"], env={"BEZ_BENCH_STUB_FAIL_RANK": "1"})
    assert r.returncode == 7, (r.returncode, r.stderr[-500:])
    assert time.time() - t0 < 120
    assert not [ln for ln in r.stdout.splitlines() if ln.startswith("{")]


def test_bench_single_rank_unchanged():
    r = _run(["--steps", "5", "--warmup", "1", "--stub-cpu"])
    assert r.returncode == 0, r.stderr
    d = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][0])
    assert d["n_gpus"] == 1


def test_bench_refuses_world_size_mismatch():
    r = _run(["--gpus", "2", "--steps", "1", "--stub-cpu"], env={"WORLD_SIZE": "1", "RANK": "0", "LOCAL_RANK": "0"})
    assert r.returncode != 0 and "WORLD_SIZE" in r.stderr


def test_bench_under_torch_distributed_run():
    """the driver's own launch form for N > 1"""
    e = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        e.pop(k, None)
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                        "--master-port", "29731", os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1", "--stub-cpu"],
                       env=e, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][0])
    assert d["n_gpus"] == 2


def test_dump_outputs_writes_every_array_or_one_seeded_sample_within_the_budget(tmp_path):
    """bench.py --dump-outputs: the arrays as given while they fit the budget; above it, the same seeded env rows of every array
    (and their ids), the same rows on every call, within the budget."""
    import numpy as np
    import bench
    n = 1000
    outs = {"obs": np.arange(n * 54, dtype=np.float32).reshape(n, 54), "reset": np.arange(n, dtype=np.float64).reshape(n, 1)}
    bench.write_outputs(outs, str(tmp_path / "all"))
    for k, a in outs.items():
        np.testing.assert_array_equal(np.load(tmp_path / "all" / (k + ".npy")), a)
    assert not (tmp_path / "all" / "env_ids.npy").exists()
    budget = 40000
    for d in ("a", "b"):
        bench.write_outputs(outs, str(tmp_path / d), budget=budget)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["env_ids.npy", "obs.npy", "reset.npy"] and sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= budget
    ids = np.load(tmp_path / "a" / "env_ids.npy")
    assert ids.dtype == np.float64 and 100 < ids.size < n and np.all(np.diff(ids) > 0)
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "reset.npy")[:, 0], ids)
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "obs.npy"), outs["obs"][ids.astype(int)])
    for f in files:
        np.testing.assert_array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f))


@pytest.mark.gpu
@pytest.mark.parametrize("launch", ["python", "c"])
def test_dump_outputs_is_the_last_timed_step(tmp_path, launch):
    """bench.py --steps K --warmup W --dump-outputs DIR: DIR holds the buffers of the (W + K)-th step of the rollout, recomputed here
    by a fresh sim on the same actions, one row per env -- and not those of the step before it.  Both launch paths."""
    import numpy as np
    import torch
    from bez_isaacgym_amd import abi
    from bez_isaacgym_amd.sim import BezSim
    n, warmup, steps, ring = 256, 3, 70, 64   # W + K past the 64-batch action ring: --launch c splits its C calls at the wrap
    r = _run(["--steps", str(steps), "--warmup", str(warmup), "--num-envs", str(n), "--launch", launch, "--no-cpu-baseline",
              "--ppo-epochs", "0", "--no-full-store", "--dump-outputs", str(tmp_path)])
    assert r.returncode == 0, r.stderr[-2000:]
    assert json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][0])["steps"] == steps
    cfg = abi.default_config(n, seed=42)
    cfg.flags |= abi.FLAG_LEAN_STEP
    sim = BezSim(cfg, 0)
    gen = torch.Generator(device=sim.device)
    gen.manual_seed(1000)
    actions = torch.rand(ring, n * 18, device=sim.device, generator=gen) * 2 - 1

    def buffers():
        out = {}
        for name, which in (("obs", abi.TENSOR_OBS), ("rew", abi.TENSOR_REW), ("reset", abi.TENSOR_RESET), ("progress", abi.TENSOR_PROGRESS),
                            ("timeout", abi.TENSOR_TIMEOUT)):
            out[name] = sim.tensor(which).cpu().numpy()
        for name, which in (("dof_target", abi.TENSOR_DOF_TARGET), ("root_state", abi.TENSOR_ROOT_STATE), ("dof_state", abi.TENSOR_DOF_STATE),
                            ("rigid_body_state", abi.TENSOR_RIGID_BODY_STATE)):
            out[name] = sim.refresh(which).cpu().numpy()
        return out
    for t in range(warmup + steps - 1):
        sim.step(actions[t % ring].contiguous())
    before = buffers()
    sim.step(actions[(warmup + steps - 1) % ring].contiguous())
    last = buffers()
    sim.close()
    assert sorted(f[:-4] for f in os.listdir(tmp_path)) == sorted(last)
    for k, a in last.items():
        d = np.load(tmp_path / (k + ".npy"))
        assert d.dtype == (np.float64 if a.dtype == np.int64 else np.float32) and d.shape == (n, a.size // n), k
        np.testing.assert_allclose(d.reshape(a.shape), a, rtol=0, atol=1e-6, err_msg=k)
    assert np.abs(np.load(tmp_path / "obs.npy") - before["obs"]).max() > 1e-3
