"""Tiny deterministic vectorised env on CPU with the VecTask step()/reset() contract, for PPO tests without a GPU; its variants with the
simulator's actuator, episode and non-finite statistics for the epoch-row tests, and a CPU agent on any of them."""
import numpy as np
import torch

from bez_isaacgym_amd import abi
from bez_isaacgym_amd.utils.config import load_config


class _Box:
    def __init__(self, n):
        self.shape = (n,)


class FakeVecEnv:
    """obs = noisy state in R^54; reward = -|a[:, :3] - tanh(state[:, :3])|^2; episodes of fixed random lengths."""

    def __init__(self, num_envs, seed=0, device="cpu", obs_dim=54, act_dim=18):
        self.n, self.obs_dim, self.act_dim, self.device = num_envs, obs_dim, act_dim, device
        self.gen = torch.Generator().manual_seed(seed)
        self.state = torch.randn(num_envs, obs_dim, generator=self.gen)
        self.t = torch.zeros(num_envs, dtype=torch.long)
        self.horizon = torch.randint(5, 40, (num_envs,), generator=self.gen)
        self.rl_device = device

    def get_env_info(self):
        return {"observation_space": _Box(self.obs_dim), "action_space": _Box(self.act_dim)}

    def reset(self):
        return {"obs": self.state.clone()}

    def step(self, actions):
        a = actions.detach().cpu()
        target = torch.tanh(self.state[:, :3])
        rew = -((a[:, :3] - target) ** 2).sum(-1) * 10.0
        self.state = 0.9 * self.state + 0.1 * torch.randn(self.n, self.obs_dim, generator=self.gen)
        self.t += 1
        done = (self.t >= self.horizon)
        timeout = done.clone()
        if done.any():
            idx = done.nonzero().squeeze(-1)
            self.state[idx] = torch.randn(len(idx), self.obs_dim, generator=self.gen)
            self.t[idx] = 0
        return {"obs": self.state.clone()}, rew, done.long(), {"time_outs": timeout.long()}


def _params(num_actors, minibatch, horizon=8, epochs=3):
    cfg = load_config(["task=bez_kick"], resolve=True)
    p = cfg["train"]["params"]
    p["config"].update(num_actors=num_actors, minibatch_size=minibatch, horizon_length=horizon, max_epochs=epochs,
                       mixed_precision=False, save_frequency=0, save_best_after=10 ** 9)
    return p


class _ActuatorFakeEnv:
    """mixin over FakeVecEnv: the env side of the actuator statistics (VecTask.dof_force_on / actuator_snapshot) with known numbers"""
    dof_force_on = True

    def actuator_snapshot(self):
        self.snapshots = getattr(self, "snapshots", 0) + 1
        n = self.n
        drive = torch.zeros(n, 18); drive[:, 0] = 100.0           # head: not a driven joint, must not count
        drive[:, 2] = 2.5; drive[:, 3] = -1.5
        status = torch.zeros(n, 18, dtype=torch.int32); status[:, 0] = 15
        status[:, 2] = abi.ACTUATOR_SATURATED_POS; status[: n // 2, 4] = abi.ACTUATOR_LOCKED_NEG
        qd = torch.zeros(n, 18); qd[:, 2] = 2.0; qd[:, 3] = 1.0   # power: 5 W on joint 2, negative (no contribution) on joint 3
        return drive, status, qd


class _CountingFakeEnv(FakeVecEnv):
    """FakeVecEnv with the simulator's episode statistics: every ended episode bumps episode_end_counts[cause, env] with a cause drawn
    from the env index and the step, and (terms on) the reward goes into slot 5 on ended steps, split over slots 0 / 2 otherwise."""

    def __init__(self, *a, terms=False, **kw):
        super().__init__(*a, **kw)
        self.episode_end_counts = torch.zeros(abi.END_CAUSES, self.n, dtype=torch.int64)
        self.reward_terms_buf = torch.zeros(abi.END_CAUSES, self.n, dtype=torch.float32)
        self.reward_terms_on = terms
        self.calls, self.ended = 0, []

    def step(self, actions):
        obs, rew, done, info = super().step(actions)
        causes = (torch.arange(self.n) + self.calls) % 3 + abi.END_FALL
        idx = done.nonzero().squeeze(-1)
        self.episode_end_counts[causes[idx], idx] += 1
        self.ended.append(done.sum().item())
        if self.reward_terms_on:
            d = done.bool()
            self.reward_terms_buf[5] += torch.where(d, rew, torch.zeros_like(rew))
            self.reward_terms_buf[0] += torch.where(d, torch.zeros_like(rew), 0.25 * rew)
            self.reward_terms_buf[2] += torch.where(d, torch.zeros_like(rew), rew - 0.25 * rew)
        self.calls += 1
        return obs, rew, done, info


class _GuardedFakeEnv(FakeVecEnv):
    """FakeVecEnv with the simulator's trip counters: `trips[k]` = {env: increments} made during the k-th step() call."""

    def __init__(self, *a, trips=None, **kw):
        super().__init__(*a, **kw)
        self.nonfinite_buf = torch.zeros(self.n, dtype=torch.int64)
        self.calls, self.trips = 0, trips or {}

    def step(self, actions):
        for e, k in self.trips.get(self.calls, {}).items():
            self.nonfinite_buf[e] += k
        self.calls += 1
        return super().step(actions)


def _agent(env, n, horizon):
    from bez_isaacgym_amd.ppo.a2c_continuous import A2CAgent
    agent = A2CAgent(_params(n, 4 * n, horizon=horizon), env, "cpu")
    agent.obs = agent.env_reset()
    return agent
