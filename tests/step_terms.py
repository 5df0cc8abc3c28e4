"""The harness of the suites that hold one term of the fused step to the fp64 oracle element by element -- ball <-> box contact
(ball_contact_ref), leg <-> leg capsules (leg_contact_ref), ground points (ground_contact_ref), joint drive, friction, limits and locks
(joint_drive_ref), external wrenches (body_wrench_ref) --, each with a CPU file (tests/test_*_cpu.py) and a GPU file (tests/test_gpu_*.py).
What they share lives here, once: the bars and the outlier budget, the config, setters and outputs of one control step, the reference
recipe (`reference`, `oracle_pair`, `step_pair`), the bar rule (`case_bars`), the comparison rule (`compare`), the report words and the
HIP side of a case.  A term module holds its geometry, state generators, `kept`, cases, planted slips and term-specific assertions."""
import os
from types import SimpleNamespace

import numpy as np

from bez_isaacgym_amd import abi
from tests.parity_util import EnvOutliers

ASSETS = {"default": 0, "cleats": abi.FLAG_CLEATS, "box": abi.FLAG_BOX_ASSET}
# the project's single-step bars (tests/test_gpu_parity.py): quantity -> (atol, rtol)
BARS = {"pose": (2e-5, 0.0), "root_vel": (4e-3, 0.0), "ball_lin": (4e-3, 0.0), "ball_spin": (4e-3, 0.0), "q": (1.5e-4, 0.0),
        "qd": (1.5e-2, 0.0), "cf": (0.04, 0.01), "imu": (1.5e-2, 0.0), "rew": (2e-5, 0.0)}
QUANTITIES = tuple(BARS)
OUTLIER_BUDGET = 3   # tests.parity_util.EnvOutliers' default budget for one step of up to 2000 envs
NEIGHBOUR_ENVS = (0, 15, 16, 63, 64, 127, 191, 192, 199)   # first / last lanes of the 16- and 64-env workgroups, and the last env
N = 1000             # a multiple of neither the 16-env nor the 64-env workgroup
KERNELS = ["ws8", "ws8q", "lane"]


# ---------------------------------------------------------------------------------------------------------------- one control step
def step_cfg(n, asset, gravity=True, substeps=2, flags=0, seed=17):
    cfg = abi.default_config(n, seed=seed)
    cfg.flags |= ASSETS[asset] | flags
    cfg.substeps = substeps
    if not gravity:
        cfg.gravity[:] = [0.0, 0.0, 0.0]
    return cfg


def dr_params(n, seed):
    """per-env friction, Kp and Kd scales (the friction feeds the contacts)"""
    rng = np.random.default_rng(seed)
    return {abi.PARAM_FRICTION: rng.uniform(0.7, 1.3, (n, 1)).astype(np.float32),
            abi.PARAM_KP_SCALE: rng.uniform(0.5, 1.5, (n, 18)).astype(np.float32),
            abi.PARAM_KD_SCALE: rng.uniform(0.5, 1.5, (n, 18)).astype(np.float32)}


def actions(n, seed):
    return np.random.default_rng(seed).uniform(-1, 1, (n, 18)).astype(np.float32)


def inject(sim, states, params=None):
    """the same state through the Isaac-layout setters of an Oracle or a SimAdapter; the episode starts here"""
    n = len(states["root_states"])
    sim.set_root_states(states["root_states"].reshape(-1, 13))
    sim.set_dof_state(states["dof_state"].reshape(-1, 2))
    sim.set_reset(np.zeros(n, np.int64)); sim.set_progress(np.zeros(n, np.int64))
    for k, v in (params or {}).items():
        sim.set_env_params(k, v)


_inject = inject   # hip_sim's argument of the same name hides the function there


def outputs(sim, n):
    """everything one step produces, per env; a task without a ball reports zeros for it"""
    rs = sim.root_states.reshape(n, -1, 13).astype(np.float64)
    ball = rs[:, 1] if rs.shape[1] > 1 else np.zeros((n, 13))
    ds = sim.dof_state.reshape(n, 18, 2).astype(np.float64)
    return dict(pose=rs[:, :, 0:7].reshape(n, -1), root_vel=rs[:, 0, 7:13], ball_lin=ball[:, 7:10], ball_spin=ball[:, 10:13],
                q=ds[:, :, 0], qd=ds[:, :, 1], cf=sim.contact_forces.reshape(n, -1).astype(np.float64),
                imu=sim.obs[:, 36:44].astype(np.float64), rew=sim.rew.reshape(n, 1).astype(np.float64),
                reset=sim.reset_buf.copy())


def env_errors(got, ref, excess=False):
    """per quantity the largest |got - ref| of every env (inf for a non-finite env); excess=True: beyond the bar's relative part,
    |got - ref| - rtol |ref|, which is what the bar's absolute part is compared with"""
    out = {}
    for k in QUANTITIES:
        err = np.abs(got[k] - ref[k]) - (BARS[k][1] * np.abs(ref[k]) if excess else 0.0)
        out[k] = np.where(np.isfinite(got[k]).all(1), err.max(1), np.inf)
    return out


def robot_momentum(sim, n, asset):
    """(linear momentum (n, 3) of the robot from the rigid-body rows and the URDF masses (as tests/scenarios.body_momenta), angular
    momentum (n, 3) about its centre of mass from the root and DOF state and the URDF masses and inertias (tests/centroidal_numpy.cm_ref))"""
    from tests import centroidal_numpy as CM
    from tests import dynamics_numpy as D
    f = np.float64
    links = D.model_of(asset)["links"]
    mass = np.array([L["mass"] for L in links]); com = np.array([L["com"] for L in links]); body = np.array([L["body"] for L in links])
    rows = sim.rigid_body_states.reshape(n, -1, 13).astype(f)[:, body]
    rc = np.einsum("nlij,lj->nli", CM._quat_to_mat(rows[..., 3:7].reshape(-1, 4), f).reshape(n, -1, 3, 3), com)
    vc = rows[..., 7:10] + np.cross(rows[..., 10:13], rc)
    lin = (mass[None, :, None] * vc).sum(1)
    root = sim.root_states.reshape(n, -1, 13)[:, 0].astype(f)
    dof = sim.dof_state.reshape(n, 18, 2).astype(f)
    E, r, a, m, c, I = CM._configuration(links, root[:, 3:7], dof[:, :, 0], np.ones((n, len(links))), f)
    centre = sum(m[i][:, None] * c[i] for i in range(len(links))) / sum(m)[:, None]
    w, v = CM._velocities(links, r, a, c, root[:, 7:10], root[:, 10:13], dof[:, :, 1])
    _, ang, _ = CM._momentum(m, c, I, w, v, centre, f)
    return lin, ang


# ---------------------------------------------------------------------------------------------------------------- the oracle's side of a case
_REFERENCES = {}


def reference(key, build, **fields):
    """The reference of a case, computed once per process and shared by every kernel's test: a namespace of `fields` that build(ref)
    fills -- cfg (a function), states, params, actions and the term's own fields, the two oracles through oracle_pair and step_pair."""
    if key not in _REFERENCES:
        ref = SimpleNamespace(**fields)
        build(ref)
        _REFERENCES[key] = ref
    return _REFERENCES[key]


def oracle_pair(ref, cfg=None, params=False):
    """the fp64 oracle and its fp32 build in the case's start state (cfg, params: another config and other parameters than the case's,
    for a planted slip); what a term measures before the step, it measures on these"""
    from oracle.bez_oracle import Oracle
    cfg = ref.cfg() if cfg is None else cfg
    pair = Oracle(cfg), Oracle(cfg, precision="f32")
    for o in pair:
        inject(o, ref.states, ref.params if params is False else params)
    return pair


def step_pair(ref, o64, o32):
    """one control step of both: ref.out64, ref.out32 and the fp32 build's own error ref.err32"""
    for o in (o64, o32):
        o.step(ref.actions)
    ref.out64, ref.out32 = outputs(o64, ref.n), outputs(o32, ref.n)
    ref.err32 = env_errors(ref.out32, ref.out64)


def case_bars(ref):
    """The bars of a case: the project's single-step bars (BARS) where the oracle's own fp32 build, on this case's kept envs, stays under
    half of one; where it does not, 3 x the fp32 build's worst error against fp64 -- measured on the oracle, never on a kernel.  The
    fp32 build flips a branch next to a switch as any fp32 implementation does (tests/parity_util.py), so its worst is taken outside the
    same OUTLIER_BUDGET envs that the kernel is allowed.  Returns quantity -> (atol, rtol, that fp32 worst)."""
    out = {}
    excess = env_errors(ref.out32, ref.out64, excess=True)
    for k, (atol, rtol) in BARS.items():
        worst = float(np.sort(excess[k][ref.kept])[-1 - OUTLIER_BUDGET])
        out[k] = (atol if worst <= 0.5 * atol else 3.0 * worst, rtol, worst)
    return out


def compare(case, ref, out, label, report=None, p99=True, also_outliers=None, elements=None):
    """The kept envs of one stepped simulator against the fp64 oracle: every env inside case_bars with EnvOutliers' default budget, reset
    flags equal outside the outliers, per quantity the p99 of |got - f64| at most 2.5 x the fp32 build's + 1e-6 (p99=False: printed
    only -- the 200-env cases, whose p99 rests on three envs), then the term's own per-element checks.
    also_outliers: (n,) bool, kept envs the term itself finds beyond a bar of its own; they count against the same budget.
    elements(bars, outlier mask) -> (further arguments of report, [(what, figure, bar), ...]): the term's per-element figures; each must
    be finite and within its bar, which is asserted last.
    report: a function that receives (errors per quantity, number of outliers, bars, *elements' arguments) before anything is asserted.
    -> the mask of the outlier envs"""
    k = ref.kept
    T = EnvOutliers(ref.n)
    assert max(T.floor, int(np.ceil(T.share * ref.n))) == OUTLIER_BUDGET
    bars = case_bars(ref)
    for q in QUANTITIES:
        atol, rtol, _ = bars[q]
        print("%s %s %-9s bar %.1e + %g%s: fp32 build %.2e" % (case, label, q, atol, rtol,
                                                               "" if atol == BARS[q][0] else " (raised: 3 x the fp32 build)", bars[q][2]))
        T.close(out[q], ref.out64[q], atol, rtol=rtol, what=q, rows=k)
    if also_outliers is not None:
        T.mark(k & also_outliers)
    bad = T.marked()
    err = env_errors(out, ref.out64)
    more, checks = elements(bars, bad) if elements is not None else ((), [])
    if report is not None:
        report(err, int(bad.sum()), bars, *more)
    T.end_step(); T.finish()
    np.testing.assert_array_equal(out["reset"][k & ~bad], ref.out64["reset"][k & ~bad])
    for q in QUANTITIES:
        h, c = np.quantile(err[q][k], 0.99), np.quantile(ref.err32[q][k], 0.99)
        print("%s %s %-9s p99 %.2e, fp32 build %.2e" % (case, label, q, h, c))
        assert not p99 or h <= 2.5 * c + 1e-6, (case, label, q, h, c)
    for what, figure, bar in checks:
        assert np.isfinite(figure) and figure <= bar, (case, label, what, figure, bar)
    return bad


def aimed_cf_checks(ref, out, bars, bad, count, what):
    """elements' checks of a contact suite: per aimed element (pair, point) the worst contact-force error, beyond the cf bar's relative
    part, of its kept envs outside the outliers, against the cf bar's absolute part"""
    atol, rtol, _ = bars["cf"]
    excess = np.abs(out["cf"] - ref.out64["cf"]) - rtol * np.abs(ref.out64["cf"])
    envs = [ref.kept & ~bad & (ref.aim == p) for p in range(count)]
    return [("%s %d" % (what, p), excess[e].max(), atol) for p, e in enumerate(envs) if e.any()]


# ---------------------------------------------------------------------------------------------------------------- reports
def error_table(ref):
    """{quantity: (worst, p99)} of the oracle's fp32 build against fp64 over the kept envs: the yardstick of the GPU file"""
    return {q: (float(ref.err32[q][ref.kept].max()), float(np.quantile(ref.err32[q][ref.kept], 0.99))) for q in QUANTITIES}


def report_words(name, width, ref, err, outliers, bars=None):
    """the common words of a report line: the name in `width` columns with the kept / outlier counts, per quantity worst / p99 of the
    kernel | of the fp32 build and, given the bars, the raised ones last"""
    k = ref.kept
    words = ["%-*s kept=%d/%d outliers=%d/%d" % (width, name, k.sum(), ref.n, outliers, OUTLIER_BUDGET)]
    for q in QUANTITIES:
        h, c = err[q][k], ref.err32[q][k]
        words.append("%s=%.1e/%.1e|%.1e/%.1e" % (q, h.max(), np.quantile(h, 0.99), c.max(), np.quantile(c, 0.99)))
    if bars is not None:
        raised = ["%s->%.1e" % (q, bars[q][0]) for q in QUANTITIES if bars[q][0] != BARS[q][0]]
        words.append("raised=%s" % (",".join(raised) or "none"))
    return words


def note(env_var, text):
    """append a line to the report file that the environment variable names, if it names one"""
    path = os.environ.get(env_var)
    if path:
        with open(path, "a") as f:
            f.write(text + "\n")


# ---------------------------------------------------------------------------------------------------------------- the HIP side of a case
def hip_sim(ref, kernel, monkeypatch, flags=0, inject=True):
    """the HIP sim of a case on `kernel` (None: the one the library selects), in the case's start state unless inject=False"""
    from tests.sim_adapter import SimAdapter
    if kernel is None:
        monkeypatch.delenv("BEZ_SIM_KERNEL", raising=False)
    else:
        monkeypatch.setenv("BEZ_SIM_KERNEL", kernel)   # read once, at bez_sim_create
    cfg = ref.cfg()
    cfg.flags |= flags
    g = SimAdapter(cfg)
    if inject:
        _inject(g, ref.states, ref.params)
    return g


def step_outputs(g, ref, health=True):
    """one control step; health: the health word must stay clear (no non-finite env, no spin wait that gave up)"""
    g.step(ref.actions)
    out = outputs(g, ref.n)
    if health:
        assert g.sim.health() == 0, g.sim.health()
    return out
