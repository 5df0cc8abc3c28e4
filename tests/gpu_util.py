"""Device helpers the GPU tests and the digest tool share: simulations of every asset, host <-> device copies, the state writer, the
per-field bars of the rigid-body rows and of the Jacobian (_J_refs), the seeded states, udot and parameter rows of the inverse- and
forward-dynamics tests (_states / _prepared; tools/dynamics_digests.py digests what the queries write on exactly these), an oracle /
HIP pair on one config (_pair), a SimAdapter on a named step kernel (_adapter), the randomisation config of the DR tests (_dr_cfg),
and the PPO agent on the HIP simulator (_agent).  Importing this initialises no GPU."""
import numpy as np
import torch

from bez_isaacgym_amd import abi
from tests import dynamics_numpy as D
from tests.sim_cfg import make_cfg
from tests.state_sets import FIELDS, ball_states, generate_states, ulp32

ASSETS = {"default": {}, "cleats": dict(cleats=True), "box": dict(box=True)}
NMAX = 300          # envs of the _states() set: the largest size of the inverse- and forward-dynamics tests
NG = abi.NUM_GEN
_CACHE = {}


def _sim(cfg):
    from bez_isaacgym_amd.sim import BezSim
    return BezSim(cfg, 0)


def _dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to("cuda:0").reshape(-1).contiguous()


def _ids(a):
    return torch.as_tensor(np.asarray(a, np.int64).astype(np.int32)).to("cuda:0").contiguous()


def _host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy().copy()


def _write_states(sim, root, dof, ball):
    n, nact = sim.num_envs, sim.num_actors
    rs = np.zeros((n, nact, 13), np.float32)
    rs[:, 0] = root
    if nact == 2:
        rs[:, 1] = ball
    sim.set_actor_root_state_tensor_indexed(_dev(rs), _ids(np.arange(n * nact)))
    sim.set_dof_state_tensor_indexed(_dev(dof), _ids(np.arange(0, n * nact, nact)))
    return rs


def _bars(err32, ref):
    """per field: 3x the fp32 oracle's worst error on these states + 2 fp32 ulps of the value (elementwise)"""
    return {name: 3.0 * float(err32[name].max()) + 2.0 * ulp32(ref[..., sl]) for name, sl in FIELDS}


def _states():
    if "states" not in _CACHE:
        root, dof, _ = generate_states(NMAX)
        rng = np.random.default_rng(29)
        # udot of O(10) in mixed SI units: m/s^2, rad/s^2
        udot = rng.uniform(-10, 10, (NMAX, NG)).astype(np.float32)
        scale = rng.uniform(0.5, 1.5, (NMAX, 19)).astype(np.float32)
        gravity = (np.array([0.0, 0.0, -9.81]) + rng.uniform(-2, 2, (NMAX, 3))).astype(np.float32)
        _CACHE["states"] = dict(root=root, dof=dof, ball=ball_states(NMAX), udot=udot, scale=scale, gravity=gravity)
    return _CACHE["states"]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _prepared(cfg, n, randomized):
    st = _states()
    sim = _sim(cfg)
    _write_states(sim, st["root"][:n], st["dof"][:n], st["ball"][:n])
    if randomized:
        sim.set_env_params(abi.PARAM_MASS_SCALE, _dev(st["scale"][:n]))
        sim.set_env_params(abi.PARAM_GRAVITY, _dev(st["gravity"][:n]))
    return sim, _dev(st["udot"][:n]).view(n, NG)


def _free():
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info(0)[0]


def _agent(num_envs, minibatch, randomize=False, **cfg_over):
    from bez_isaacgym_amd.ppo.a2c_continuous import A2CAgent
    from bez_isaacgym_amd.utils.config import load_config
    from bez_isaacgym_amd.utils.rlgames_utils import RLGPUEnv, get_rlgames_env_creator
    args = ["task=bez_kick", "num_envs=%d" % num_envs, "headless=True"] + (["task.task.randomize=True"] if randomize else [])
    cfg = load_config(args)
    cfg["task"]["seed"] = 42
    creator = get_rlgames_env_creator(cfg["task"], "bez_kick", "cuda:0", "cuda:0", 0, True)
    venv = RLGPUEnv("rlgpu", num_envs, env_creator=creator)
    params = cfg["train"]["params"]
    params["config"].update(minibatch_size=minibatch, save_frequency=0, save_best_after=10 ** 9, **cfg_over)
    return A2CAgent(params, venv, "cuda:0")


def _pair(n, **kw):
    from oracle.bez_oracle import Oracle
    from tests.sim_adapter import SimAdapter
    return Oracle(abi.default_config(n, **kw)), SimAdapter(abi.default_config(n, **kw))


def _adapter(cfg, kernel, monkeypatch):
    from tests.sim_adapter import SimAdapter
    monkeypatch.setenv("BEZ_SIM_KERNEL", kernel)
    return SimAdapter(cfg)


def _dr_cfg(freq=5, sched=40):
    r = lambda a, b, s=sched: {"range": [a, b], "schedule": "linear", "schedule_steps": s}
    return abi.dr_config_from_params({
        "frequency": freq,
        "observations": {"range": [0, .002], "operation": "additive", "distribution": "gaussian"},
        "actions": {"range": [0., .02], "operation": "additive", "distribution": "gaussian", "schedule": "linear", "schedule_steps": sched},
        "sim_params": {"gravity": dict(r(0, 0.4), operation="additive", distribution="gaussian")},
        "actor_params": {"bez": {
            "rigid_shape_properties": {"friction": dict(r(0.7, 1.3), num_buckets=500, operation="scaling", distribution="uniform")},
            "dof_properties": {"damping": dict(r(0.5, 1.5), operation="scaling", distribution="uniform"),
                               "stiffness": dict(r(0.5, 1.5), operation="scaling", distribution="uniform"),
                               "lower": dict(r(0, 0.01), operation="additive", distribution="gaussian"),
                               "upper": dict(r(0, 0.01), operation="additive", distribution="gaussian")}}}})


def _J_refs(asset, root, dof, key):
    """(fp64 J_ref, per-field bars) of an asset from the oracle's unit-velocity rows; computed once per key and left unchanged"""
    if key not in _CACHE:
        cfg = lambda n: make_cfg(n, task="bez_walk", seed=5, **ASSETS[asset])
        nb = 29 if asset == "cleats" else 21
        J64 = D.J_ref_oracle(cfg, "f64", root, dof, nb)
        J32 = D.J_ref_oracle(cfg, "f32", root, dof, nb)
        err32 = np.abs(J32 - J64)
        bars = np.empty_like(J64)
        for sl in (slice(0, 3), slice(3, 6)):
            bars[:, :, sl] = 3.0 * float(err32[:, :, sl].max()) + 2.0 * ulp32(J64[:, :, sl])
        _CACHE[key] = (J64, bars)
    return _CACHE[key]


DEV = "cuda"
SENT = 7.0      # sentinel of every output buffer (an fp16 number; no case produces a tensor of sevens)
GUARD = 3       # sentinel rows behind row n


class Guarded:
    """(n, cols) output filled with the sentinel, with GUARD more sentinel rows behind it"""

    def __init__(self, n, cols=None, dtype=torch.float32):
        self.n = n
        self.full = torch.full((n + GUARD,) if cols is None else (n + GUARD, cols), SENT, device=DEV, dtype=dtype)
        self.t = self.full[:n]

    def band_untouched(self):
        return bool((self.full[self.n:] == SENT).all())

    def untouched(self):
        return bool((self.full == SENT).all())

    def np(self):
        return self.t.double().cpu().numpy()
