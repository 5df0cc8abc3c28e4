"""CPU: the PPO consumer loop (rl_games a2c_continuous semantics) -- shapes, GAE against a literal restatement, learning
on a toy env, checkpoint key layout, and the multi-process path on gloo (world_size 2)."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from bez_isaacgym_amd.ppo.a2c_continuous import (A2CAgent, ModelA2CContinuousLogStd, RunningMeanStd, discount_values)
from bez_isaacgym_amd.utils.config import load_config
from tests.fake_env import FakeVecEnv, _params


def test_network_matches_reference_checkpoint_shapes():
    """54-400-200-100 ELU trunk, mu 18, sigma 18, value 1: 124 237 parameters (Bez_Kick_33.pth / bez_kickPPO.yaml:25-27)."""
    m = ModelA2CContinuousLogStd(54, 18, (400, 200, 100))
    sd = m.state_dict()
    assert sum(v.numel() for v in sd.values()) == 124237
    expect = {"a2c_network.sigma": (18,), "a2c_network.actor_mlp.0.weight": (400, 54), "a2c_network.actor_mlp.2.weight": (200, 400),
              "a2c_network.actor_mlp.4.weight": (100, 200), "a2c_network.value.weight": (1, 100), "a2c_network.mu.weight": (18, 100)}
    for k, shp in expect.items():
        assert tuple(sd[k].shape) == shp, k


def test_gae_matches_literal_definition():
    torch.manual_seed(0)
    H, N = 7, 5
    rew, val = torch.randn(H, N, 1), torch.randn(H, N, 1)
    dones = (torch.rand(H, N) < 0.2).float()
    last_v, last_d = torch.randn(N, 1), (torch.rand(N) < 0.2).float()
    adv = discount_values(0.99, 0.95, last_d, last_v, dones, val, rew)
    ref = torch.zeros(H, N)
    for n in range(N):
        gae = 0.0
        for t in reversed(range(H)):
            nd = last_d[n] if t == H - 1 else dones[t + 1, n]
            nv = last_v[n, 0] if t == H - 1 else val[t + 1, n, 0]
            delta = rew[t, n, 0] + 0.99 * nv * (1 - nd) - val[t, n, 0]
            gae = delta + 0.99 * 0.95 * (1 - nd) * gae
            ref[t, n] = gae
    np.testing.assert_allclose(adv.squeeze(-1).numpy(), ref.numpy(), atol=1e-5)


def test_running_mean_std_matches_numpy():
    rms = RunningMeanStd((3,))
    rng = np.random.default_rng(0)
    chunks = [rng.normal(2.0, 3.0, (100, 3)), rng.normal(-1.0, 0.5, (50, 3))]
    rms.train()
    for c in chunks:
        rms(torch.from_numpy(c).float())
    allx = np.concatenate(chunks)
    # rl_games starts from count=1 (a virtual sample at mean 0, var 1): reproduce
    n = len(allx)
    mean = allx.sum(0) / (n + 1)
    np.testing.assert_allclose(rms.running_mean.numpy(), mean, rtol=1e-5)
    assert abs(float(rms.count) - (n + 1)) < 1e-9


def test_learns_toy_env_and_checkpoint_roundtrip(tmp_path):
    env = FakeVecEnv(64, seed=1)
    agent = A2CAgent(_params(64, 256, horizon=8), env, "cpu")
    agent.obs = agent.env_reset()
    first = [agent.train_epoch() for _ in range(3)]
    r0 = float(np.mean(agent.game_rewards)) if agent.game_rewards else None
    for _ in range(40):
        agent.train_epoch()
    r1 = float(np.mean(agent.game_rewards))
    assert r0 is None or r1 > r0, (r0, r1)
    state = agent.get_full_state_weights()
    assert {"model", "running_mean_std", "reward_mean_std", "optimizer", "epoch", "frame", "last_mean_rewards"} <= set(state)
    assert set(state["running_mean_std"]) == {"running_mean", "running_var", "count"} and state["running_mean_std"]["running_mean"].dtype == torch.float64
    path = str(tmp_path / "ck.pth")
    agent.save(path)
    other = A2CAgent(_params(64, 256, horizon=8), FakeVecEnv(64, seed=1), "cpu")
    other.restore(path)
    for a, b in zip(agent.model.parameters(), other.model.parameters()):
        assert torch.equal(a, b)
    assert other.epoch_num == agent.epoch_num and other.frame == agent.frame


def test_epoch_report_layout_is_pinned_and_grows_with_mini_epochs():
    """EpochReport: for mini_epochs <= 68 the offsets and the 64-word size are the ones every earlier version used; beyond, the fields behind
    the KL accumulators move up -- no two fields share a byte, every field lies inside the buffer -- and the epoch row keeps its keys."""
    from bez_isaacgym_amd import abi
    from bez_isaacgym_amd.ppo.a2c_continuous import EpochReport
    names = ("ep_stats", "lr", "loss", "kl", "actuators", "episode_ends", "reward_terms", "nonfinite", "health")
    for me in (1, 5, 68, 69, 200):
        lay = EpochReport(me)
        assert tuple(lay.fields) == names
        assert [lay.fields[k][2] for k in names] == [3, 1, 2, me, 4, abi.END_CAUSES, abi.REWARD_TERM_SLOTS, 1, 1]
        assert [lay.fields[k][0] for k in names] == [torch.float64] + 3 * [torch.float32] + 5 * [torch.float64]
        if me <= 68:
            assert [lay.fields[k][1] for k in names] == [0, 8, 10, 12, 40, 46, 54, 62, 63] and lay.words == 64
        spans = sorted((o * t.itemsize, (o + n) * t.itemsize) for t, o, n in lay.fields.values())
        assert spans[0][0] == 0 and spans[-1][1] <= 8 * lay.words
        assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), (me, spans)
        assert lay.fields["loss"][1] + 2 == lay.fields["kl"][1]     # neighbours: one fill zeroes both
        # the same through the views the trainer uses: a mark written into every field survives the writes into all the others
        buf = torch.zeros(lay.words, dtype=torch.float64)
        for i, k in enumerate(names):
            assert lay.view(buf, k).numel() == lay.fields[k][2]
            lay.view(buf, k).fill_(i + 1)
        assert all((lay.view(buf, k) == i + 1).all() for i, k in enumerate(names))
        assert lay.view(buf, "loss", "kl").numel() == 2 + me

    from tests.fake_env import _ActuatorFakeEnv, _CountingFakeEnv, _GuardedFakeEnv

    class _Actuators(_ActuatorFakeEnv, FakeVecEnv):
        pass
    for make in (lambda: _GuardedFakeEnv(16, seed=7, trips={2: {3: 1}}), lambda: _CountingFakeEnv(16, seed=7, terms=True),
                 lambda: _Actuators(16, seed=7)):
        rows = {}
        for me in (5, 69):
            p = _params(16, 64, horizon=4)
            p["config"]["mini_epochs"] = me
            agent = A2CAgent(p, make(), "cpu")
            assert agent._report.numel() == (64 if me == 5 else 65) and agent.kl_acc.numel() == me
            agent.obs = agent.env_reset()
            rows[me] = [agent.train_epoch() for _ in range(2)]
        assert all(set(a) == set(b) for a, b in zip(rows[5], rows[69])), (sorted(rows[5][0]), sorted(rows[69][0]))
        a, b = rows[5][0], rows[69][0]   # the first rollout does not depend on the update: the same numbers, wherever the fields lie
        for k in ("nonfinite_resets", "sim_health", "episode_ends", "reward_terms", "actuators"):
            assert a.get(k) == b.get(k), k
    assert rows[5][0]["actuators"] and "episode_ends" not in rows[5][0]


def _dp_worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.set_num_threads(1)
    env = FakeVecEnv(32, seed=100 + rank)           # each rank owns its own envs (sharded, no data-path collective)
    agent = A2CAgent(_params(32, 128, horizon=8), env, "cpu", rank=rank, world=world)
    agent.obs = agent.env_reset()
    for _ in range(3):
        agent.train_epoch()
    flat = torch.cat([p.detach().reshape(-1) for p in agent.model.parameters()])
    out[rank] = (flat.clone(), agent.running_mean_std.running_mean.clone(), agent.last_lr, agent.frame)
    # SURVEY.md 5.8 / VERDICT round 2 item 5: collectives of ONE more epoch = 2 for the epoch's data-only moments + 1 per optimiser step
    calls = []
    real = dist.all_reduce
    dist.all_reduce = lambda t, *a, **k: (calls.append(int(t.numel())), real(t, *a, **k))[1]
    try:
        agent.train_epoch()
    finally:
        dist.all_reduce = real
    out["calls%d" % rank] = (calls, agent.mini_epochs * agent.num_minibatches)
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_data_parallel_gloo_world2_replicas_stay_identical():
    """One process per rank, gradient all-reduce per optimiser step: after training on DIFFERENT env shards both replicas
    hold bit-identical parameters, identical input statistics and the same adaptive LR; frames count the whole job."""
    mgr = mp.Manager()
    out = mgr.dict()
    port = 29500 + (os.getpid() % 2000)
    mp.spawn(_dp_worker, args=(2, port, out), nprocs=2, join=True)
    (p0, m0, lr0, f0), (p1, m1, lr1, f1) = out[0], out[1]
    assert torch.equal(p0, p1)
    assert torch.equal(m0, m1)
    assert lr0 == lr1 and f0 == f1 == 3 * 8 * 32 * 2
    calls, steps = out["calls0"]
    assert out["calls1"][0] == calls
    assert len(calls) == steps + 2, calls            # one collective per optimiser step + two per epoch (was two per step + three)
    nparam = p0.numel()
    assert calls[2:] == [nparam + 1] * steps         # gradient + KL in one message
    assert calls[1] == 6                             # advantage moments + episode statistics


def test_restore_foreign_checkpoint_never_unpickles(tmp_path):
    """rl_games writes numpy scalars into its checkpoints (the reference's Bez_Kick_33.pth does): torch's weights_only loader
    refuses them.  restore() must then read the file with the no-unpickle reader, not fall back to a full unpickle."""
    src = A2CAgent(_params(16, 64, horizon=4), FakeVecEnv(16, seed=3), "cpu")
    state = src.get_full_state_weights()
    state["last_mean_rewards"] = np.float32(12.5)   # numpy.core.multiarray.scalar in the pickle, as rl_games does
    del state["optimizer"], state["scaler"]
    path = str(tmp_path / "foreign.pth")
    torch.save(state, path)
    with pytest.raises(Exception):
        torch.load(path, weights_only=True)
    dst = A2CAgent(_params(16, 64, horizon=4), FakeVecEnv(16, seed=4), "cpu")
    for p in dst.model.parameters():
        p.data.add_(1.0)
    dst.restore(path)
    for a, b in zip(src.model.parameters(), dst.model.parameters()):
        assert torch.equal(a, b)
    assert abs(dst.last_mean_rewards - 12.5) < 1e-6


def _amp_worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.set_num_threads(1)
    agent = A2CAgent(_params(32, 128, horizon=8), FakeVecEnv(32, seed=200 + rank), "cpu", rank=rank, world=world)
    agent.scaler = torch.amp.GradScaler("cpu", enabled=True, init_scale=1024.0, growth_interval=10 ** 6)  # AMP bookkeeping on CPU
    agent.obs = agent.env_reset()
    before = torch.cat([p.detach().reshape(-1) for p in agent.model.parameters()]).clone()
    if rank == 1:  # an fp16-style overflow on ONE rank only, on the first optimiser step
        fired = []
        p0 = next(agent.model.parameters())
        def poison(g):
            if not fired:
                fired.append(1)
                return torch.full_like(g, float("inf"))
            return g
        p0.register_hook(poison)
    agent.play_steps()
    agent.calc_gradients(agent._minibatch(0), torch.zeros(()), torch.zeros(2))
    after1 = torch.cat([p.detach().reshape(-1) for p in agent.model.parameters()]).clone()
    scale1 = float(agent.scaler.get_scale())
    agent.calc_gradients(agent._minibatch(1), torch.zeros(()), torch.zeros(2))
    after2 = torch.cat([p.detach().reshape(-1) for p in agent.model.parameters()]).clone()
    out[rank] = (before, after1, after2, scale1)
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_amp_overflow_on_one_rank_skips_the_step_everywhere():
    """Mixed precision + data parallel: the scaled gradients are all-reduced BEFORE unscale_, so an overflow on one rank
    makes every rank skip that optimiser step and back off its loss scale together; the replicas stay bit-identical and finite."""
    mgr = mp.Manager()
    out = mgr.dict()
    port = 31500 + (os.getpid() % 2000)
    mp.spawn(_amp_worker, args=(2, port, out), nprocs=2, join=True)
    (b0, a0, c0, s0), (b1, a1, c1, s1) = out[0], out[1]
    assert torch.equal(b0, b1)
    assert torch.equal(a0, b0) and torch.equal(a1, b1)      # step 1 skipped on BOTH ranks
    assert s0 == s1 == 512.0                                # both backed off 1024 -> 512
    assert torch.equal(c0, c1) and not torch.equal(c0, a0)  # step 2 taken, identically
    assert torch.isfinite(c0).all()


def _cli_worker(rank, world, port, out, tmp):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world))
    os.chdir(tmp)
    torch.set_num_threads(1)
    from bez_isaacgym_amd.train import launch
    seen = {}

    def factory(task_cfg, r):
        seen.update(rank=task_cfg.get("rank"), offset=task_cfg.get("env_id_offset"), n=task_cfg["env"]["numEnvs"])
        return FakeVecEnv(int(task_cfg["env"]["numEnvs"]), seed=300 + r)
    res = launch(["task=bez_kick", "num_envs=32", "headless=True", "multi_gpu=True", "max_iterations=2",
                  "train.params.config.minibatch_size=128", "train.params.config.horizon_length=8",
                  "train.params.config.mixed_precision=False", "train.params.config.save_frequency=0"], vec_env_factory=factory)
    out[rank] = (seen, res[1], os.path.exists(os.path.join(tmp, "runs")))


@pytest.mark.timeout(300)
def test_train_cli_multi_gpu_wiring_on_gloo(tmp_path, monkeypatch):
    """`train.py task=bez_kick multi_gpu=True` under torch.distributed.run's environment (rlgames_utils.py:71-81, config.yaml:40):
    process group, rank -> env shard (global env-id offset = rank * num_envs), data-parallel agent, rank-0-only run directory."""
    mgr = mp.Manager()
    out = mgr.dict()
    port = 33500 + (os.getpid() % 2000)
    # the workers see no GPU, so launch() takes its gloo path on every box (on a 1-GPU box RCCL would hand rank 1 a missing device)
    monkeypatch.setenv("HIP_VISIBLE_DEVICES", "")
    monkeypatch.setenv("CUDA_VISIBLE_DEVICES", "")
    mp.spawn(_cli_worker, args=(2, port, out, str(tmp_path)), nprocs=2, join=True)
    assert out[0][0] == {"rank": 0, "offset": 0, "n": 32} and out[1][0] == {"rank": 1, "offset": 32, "n": 32}
    assert out[0][1] == out[1][1] == 2


def test_cli_config_contract():
    """train.py's CLI contract: task=bez_kick num_envs=... sim_device=... pipeline=... headless=... (README.md:46-63)."""
    cfg = load_config(["task=bez_kick", "num_envs=64", "sim_device=cpu", "pipeline=cpu", "headless=True", "max_iterations=7"])
    assert cfg["task_name"] == "bez_kick" and cfg["task"]["env"]["numEnvs"] == 64
    assert cfg["task"]["sim"]["use_gpu_pipeline"] is False and cfg["task"]["sim"]["physx"]["use_gpu"] is False
    assert cfg["train"]["params"]["config"]["max_epochs"] == 7 and cfg["train"]["params"]["config"]["num_actors"] == 64
    assert cfg["train"]["params"]["config"]["minibatch_size"] == 32768 and cfg["train"]["params"]["config"]["horizon_length"] == 32


def test_switch_table_is_pinned_and_read_once():
    """Every A/B switch of the agent is a row of ONE table (name, default, what it does), read once in __init__: names and defaults are
    pinned here, bench.py's A/B list is a subset of it, an agent built without overrides holds every switch at its default, and no
    method behind __init__ reads a switch from the config again."""
    import inspect
    import re
    from bez_isaacgym_amd.ppo import a2c_continuous as m
    want = dict(hip_graphs="auto", lean_env_step=True, dp_capture_collectives=False, dp_direct_rccl=True, fused_ops=True, half_path=True,
                wgrad_splits=32, fused_optimizer=True, fused_policy_forward=True, packed_weights=True, fused_policy_backward=True,
                rollout_into_dataset=True, episode_sum_slots=True, fold_rollout_post=True, fold_action_noise=True, fold_dr_step=True,
                dr_prelaunch=False, fused_dataset_prep=True, fused_grad_reduce=True, fused_loss_backward=True, fused_wgrad=True,
                fused_train_forward=True, dp_grid_norm=True, dp_eager_update=False, pipeline_epochs=True)
    assert [name for name, _, _ in m.SWITCHES] == list(want) and all(isinstance(doc, str) and doc for _, _, doc in m.SWITCHES)
    for name, default, _ in m.SWITCHES:
        assert default == want[name] and type(default) is type(want[name]), name
    # bench.py's own list of A/B names, from its source text
    bench = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bench.py")).read()
    names = re.search(r'for k in \(([^)]*)\):\s*# A/B switches', bench)
    ab = re.findall(r'"(\w+)"', names.group(1))
    assert len(ab) == 9 and set(ab) <= set(want), sorted(set(ab) - set(want))
    p = _params(16, 64, horizon=4)
    assert not set(want) & set(p["config"])                     # the shipped YAML overrides none of them ...
    p["config"]["no_such_switch"] = 1                           # ... and a key the table does not know is ignored
    agent = A2CAgent(p, FakeVecEnv(16, seed=5), "cpu")
    assert vars(agent.sw) == want and agent.cfg is p["config"]
    assert m.read_switches(dict(fold_dr_step=False, dr_prelaunch=True)).__dict__ == dict(want, fold_dr_step=False, dr_prelaunch=True)
    assert not any(vars(agent.plan).values())                   # nothing of the fused path is planned on the CPU
    # source level: the config is read in __init__ alone
    for name, fn in inspect.getmembers(A2CAgent, inspect.isfunction):
        if name != "__init__":
            assert not re.search(r"\bcfg\s*\.\s*get\s*\(|\bcfg\s*\[", inspect.getsource(fn)), name
    src = inspect.getsource(m)
    assert src.count("cfg.get(") == 1 and "cfg.get(" in inspect.getsource(m.read_switches)
