"""The per-env non-finite guard (BEZ_FLAG_NONFINITE_GUARD, include/bez_sim.h) on the GPU: a NaN / inf pushed into one env's state trips
that env alone -- finite outputs, rew 0, reset_buf 1, its counter and the health bit -- the next step performs the ordinary reset, and
every other env stays bit-identical to a twin sim in which nothing went wrong.  Runs without a trip are bit-identical with the flag on
and off."""
import numpy as np
import pytest
import torch

from bez_isaacgym_amd import abi
from tests.guard_util import _actions, _assert_env_finite, _assert_others_equal, _floats, _inject, _sim, _snap, _twin

pytestmark = pytest.mark.gpu

KERNELS = ("lane", "ws8", "ws8q")


# ---- 1. physics-free: the split path's post-physics alone (one-env-per-lane kernel)
@pytest.mark.parametrize("cleats", [False, True])
def test_post_physics_trips_injected_env(monkeypatch, cleats):
    n, e = 64, 21
    A, B = _sim(monkeypatch, n, "lane", cleats), _sim(monkeypatch, n, "lane", cleats)
    rng = np.random.default_rng(1)
    for _ in range(3):
        act = _actions(rng, n)
        A.step(act); B.step(act)
    _inject(A, e, "qd", float("nan"))
    act = _actions(rng, n)
    for s in (A, B):
        s.pre_physics(act); s.post_physics()
    torch.cuda.synchronize()
    sa, sb = _snap(A), _snap(B)
    assert np.isfinite(_floats(sa[abi.TENSOR_OBS][e])).all()
    assert _floats(sa[abi.TENSOR_REW])[e, 0] == 0.0 and sa[abi.TENSOR_RESET][e, 0] == 1
    _assert_env_finite(sa, e)
    cnt = A.nonfinite_counts.cpu().numpy()
    assert cnt[e] == 1 and cnt.sum() == 1
    assert A.health() == abi.HEALTH_NONFINITE
    assert B.health() == 0 and B.nonfinite_counts.sum().item() == 0
    _assert_others_equal(sa, sb, [e])


@pytest.mark.parametrize("cleats", [False, True], ids=["default", "cleats"])
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("n,e,what,value", [(64, 40, "qd", float("nan")), (100, 0, "root", float("inf")), (100, 97, "q", float("nan")),
                                             (64, 8, "root", float("nan"))], ids=["64-mid-qd-nan", "100-e0-root-inf", "100-partial-q-nan", "64-root-nan"])
def test_twin_trip_then_ordinary_reset(monkeypatch, kernel, cleats, n, e, what, value):
    _twin(monkeypatch, n, e, kernel, cleats, what=what, value=value)


@pytest.mark.parametrize("kernel", KERNELS)
def test_twin_trip_walk_task(monkeypatch, kernel):
    _twin(monkeypatch, 64, 40, kernel, task=abi.TASK_WALK, what="qd")


@pytest.mark.parametrize("kernel", KERNELS)
def test_twin_trip_randomised(monkeypatch, kernel):
    _twin(monkeypatch, 64, 40, kernel, dr=True, what="root", value=float("-inf"))


# ---- 3. no trip: flag on and off give the same bits
@pytest.mark.parametrize("variant", ["default", "cleats", "randomised"])
@pytest.mark.parametrize("kernel", KERNELS)
def test_no_trip_is_bit_identical(monkeypatch, kernel, variant):
    n = 4096
    on, off = (_sim(monkeypatch, n, kernel, cleats=variant == "cleats", guard=g) for g in (True, False))
    if variant == "randomised":   # the DR kernels, with the observation noise in the step's copy-out
        from bez_isaacgym_amd.utils.config import load_config
        params = load_config(["task=bez_kick"], resolve=True)["task"]["task"]["randomization_params"]
        for s in (on, off):
            s.set_flags(int(s.cfg.flags) | abi.FLAG_OBS_NOISE_IN_STEP)
            s.set_randomization(abi.dr_config_from_params(params))
    off.set_flags(int(off.cfg.flags) & ~abi.FLAG_NONFINITE_GUARD | (abi.FLAG_OBS_NOISE_IN_STEP if variant == "randomised" else 0))
    rng = np.random.default_rng(9)
    for t in range(200):
        act = _actions(rng, n)
        on.step(act); off.step(act)
    torch.cuda.synchronize()
    a, b = _snap(on), _snap(off)
    for w in a:
        np.testing.assert_array_equal(a[w], b[w])
    assert on.nonfinite_counts.sum().item() == 0 and on.health() == 0 and off.health() == 0


# ---- 4. inside bez_sim_step_many and inside a captured graph's replay
def test_trip_inside_step_many(monkeypatch):
    n, e = 64, 33
    s = _sim(monkeypatch, n, "ws8q")
    rng = np.random.default_rng(2)
    s.step(_actions(rng, n))
    _inject(s, e, "qd", float("nan"))
    acts = torch.cat([_actions(rng, n) for _ in range(4)])
    s.step_many(acts, 4)
    torch.cuda.synchronize()
    cnt = s.nonfinite_counts.cpu().numpy()
    assert cnt[e] == 1 and cnt.sum() == 1
    assert s.health(clear=True) == abi.HEALTH_NONFINITE and s.health() == 0
    _assert_env_finite(_snap(s), e)


def test_trip_inside_graph_replay(monkeypatch):
    n, e = 64, 12
    s = _sim(monkeypatch, n, "ws8q")
    act = _actions(np.random.default_rng(3), n)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            s.step(act)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        s.step(act)
    g.replay()
    torch.cuda.synchronize()
    assert s.nonfinite_counts.sum().item() == 0
    _inject(s, e, "root", float("nan"))
    g.replay()
    torch.cuda.synchronize()
    cnt = s.nonfinite_counts.cpu().numpy()
    assert cnt[e] == 1 and cnt.sum() == 1 and s.health() == abi.HEALTH_NONFINITE
    g.replay()   # the ordinary reset
    torch.cuda.synchronize()
    assert s.nonfinite_counts.sum().item() == 1
    _assert_env_finite(_snap(s), e)


# ---- 5. a training run survives one bad env
def test_training_survives_a_nan_env():
    from bez_isaacgym_amd.ppo.a2c_continuous import A2CAgent
    from bez_isaacgym_amd.utils.config import load_config
    from bez_isaacgym_amd.utils.rlgames_utils import RLGPUEnv, get_rlgames_env_creator
    N = 512
    cfg = load_config(["task=bez_kick", "num_envs=%d" % N, "headless=True"])
    cfg["task"]["seed"] = 42
    venv = RLGPUEnv("rlgpu", N, env_creator=get_rlgames_env_creator(cfg["task"], "bez_kick", "cuda:0", "cuda:0", 0, True))
    params = cfg["train"]["params"]
    params["config"].update(minibatch_size=4096, save_frequency=0, save_best_after=10 ** 9)
    a = A2CAgent(params, venv, "cuda:0")
    a.obs = a.env_reset()
    rows = [a.train_epoch() for _ in range(2)]
    _inject(venv.env.sim, 77, "qd", float("nan"))
    rows += [a.train_epoch() for _ in range(2)]
    # the pipelined epochs train() runs by default report the same way
    _inject(venv.env.sim, 300, "root", float("nan"))
    ticket = a.train_epoch_launch()
    assert ticket is not None
    rows.append(a.train_epoch_finish(ticket))
    torch.cuda.synchronize()
    assert rows[4]["nonfinite_resets"] >= 1 and rows[4]["sim_health"] & abi.HEALTH_NONFINITE, rows
    assert rows[3]["nonfinite_resets"] == 0, rows
    assert rows[2]["nonfinite_resets"] >= 1, rows
    assert rows[2]["sim_health"] & abi.HEALTH_NONFINITE
    for p in a.model.parameters():
        assert torch.isfinite(p).all()
    for rms in (a.running_mean_std, a.value_mean_std):
        if rms is not None:
            assert torch.isfinite(rms.running_mean).all() and torch.isfinite(rms.running_var).all()
    assert torch.isfinite(a.ep_stats).all()
    assert all(np.isfinite([c, r, l]).all() for c, r, l in a._ep_hist)
    assert all(np.isfinite(v) for v in a.game_rewards)
