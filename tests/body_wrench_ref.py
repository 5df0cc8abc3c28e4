"""The external wrenches of the fused step (bez_sim_apply_body_forces), body by body: load patterns that aim every
rigid body row (fixed bodies, cleats and the ball's row included) in every mode of the call, magnitudes derived from the fp64 mass
matrix, the oracle's side of a case (oracle.bez_oracle.Oracle.apply_body_forces, written from DESIGN 4.3c with a pending list of
entries instead of the kernels' moment matrix), the response bars and the comparison of tests/test_body_wrench_cpu.py and
tests/test_gpu_body_wrench.py (on the harness of tests/step_terms.py).

Scenarios (`case_states`):
  flight   joint_drive_ref._base: zero gravity, floating base, root at +-0.3 m/s and +-1 rad/s, easy joints, default gains, the ball in
           the air 3 m away with a random attitude, +-0.5 m/s and a spin of U(-20, 20) rad/s per axis: its own row is a moving body
  stance   ball_contact_ref.kick_stance_states: under gravity, feet on the ground, the ball against a foot / leg box
  lying    ground_contact_ref.lying_states: torso / head / forearm points under the plane
  late     flight, where the call is made from a first state (`first`) and flight's state is injected before the step
Load patterns (`loads` -> a list of calls [F, T, X or None, space], fp32 (n, rows, 3)):
  solo     env e loads body e % rows alone, in mode (e // rows) % 4 of MODES; one call per mode
  all      every body of every env in one ENV call with points within REACH of each body's centre of mass
  stacked  three calls before one launch: ENV without points, LOCAL with points, ENV with points, each on a random third of the bodies
           and on /torso, /imu_link, /camera
  sparse   solo in NEIGHBOUR_ENVS only
Magnitudes (`_scale`): every loaded body's force and torque are first scaled so that each alone changes the fastest joint rate by
1 rad/s over one control step of the free robot -- dt M^-1 J^T w with tests/forward_dynamics_numpy.M_batch (fp64, armature in) and
tests/generalized_forces_numpy.gf_ref --, then the env's sum is scaled so that its largest predicted |dqd| is U(EASY) rad/s (`hard`:
times U(HARD)).  The ball: F dt / m = 1 m/s and T dt / I = 1 rad/s, times its own draw of the same ranges."""
from types import SimpleNamespace

import numpy as np

from bez_isaacgym_amd import abi
from tests import ball_contact_ref as B
from tests import forward_dynamics_numpy as FD
from tests import generalized_forces_numpy as GF
from tests import ground_contact_ref as G
from tests import joint_drive_ref as J
from tests import step_terms as S
from tests.step_terms import inject, outputs

N = S.N
RESPONSE = ("root_vel", "qd", "ball_lin", "ball_spin")
MODES = ("env_centre", "env_point", "local_centre", "local_point")   # *_centre: force + torque at the body's centre of mass; *_point: a force at a point
ENV, LOCAL = abi.SPACE_ENV, abi.SPACE_LOCAL
EASY = (0.3, 1.5)           # rad/s: the env's largest predicted |dqd| over the control step
HARD = (10.0, 20.0)         # times EASY.  (3, 6) left the drives unsaturated -- the implicit drive's h^2 kp + h kd = 0.07 kg m^2 stands beside link
                            # inertias of 1e-3 -- and showed a new saturation or lock bit in 0.9 % of the kept envs; (10, 20): 23 %
NUDGE = 3e-4                # m: the ground scenarios' start states are moved by multiples of this off ground_contact_ref's knife edges
REACH = 0.03                # m: points of application lie within this of the body's centre of mass, per axis
BALL_SPIN = 20.0            # rad/s
BALL_SPEED = 0.5            # m/s
GRAVITY = ("stance", "lying")
ALWAYS = ("/torso", "/imu_link", "/camera")   # loaded by every call of `stacked`: two fixed bodies of one link and the link itself
FIXED_BASE = abi.FLAG_FIX_BASE


def tables(asset, task="bez_kick"):
    """the body rows of an asset and task: robot bodies nb, rows nbe (the ball's row follows the robot's where the task has a ball),
    link, offset and centre of mass of every robot body, the rows' names"""
    m = B.model()
    t = m["cleats"] if asset == "cleats" else m
    nb, ball = int(t["num_bodies"]), task == "bez_kick"
    return SimpleNamespace(nb=nb, nbe=nb + int(ball), ball=ball, link=np.asarray(t["body_link"]), off=np.asarray(t["body_offset"], np.float64),
                           com=np.asarray(t["body_com"], np.float64), names=list(t["body_names"]) + (["ball"] if ball else []))


# ---------------------------------------------------------------------------------------------------------------- states
def flight_states(n, asset, seed=21, fixed=False):
    rng = np.random.default_rng(seed)
    rs, q, qd, target = J._base(n, asset, rng)
    quat = rng.normal(size=(n, 4))
    rs[:, 1, 3:7] = quat / np.linalg.norm(quat, axis=1, keepdims=True)
    rs[:, 1, 7:10] = rng.uniform(-BALL_SPEED, BALL_SPEED, (n, 3))
    rs[:, 1, 10:13] = rng.uniform(-BALL_SPIN, BALL_SPIN, (n, 3))
    if fixed:   # a welded torso stands still
        rs[:, 0, 7:13] = 0.0
    return J._finish(rs, q, qd, target)


def ground_kept(st, asset, cfg):
    """ground_contact_ref.kept of a start state, from the fp64 oracle's rigid-body rows"""
    from oracle.bez_oracle import Oracle
    o = Oracle(cfg)
    inject(o, st)
    return G.kept(G.terms(st, asset, o.rigid_body_states.reshape(len(st["root_states"]), -1, 13), cfg))


def _off_the_ground_edges(st, asset):
    """st with robot and ball moved together, up or down by up to three NUDGEs, in the envs in which a ground point (the ball's
    included: kick_stance_states rests it 0 - 2 mm deep) starts within ground_contact_ref.KEPT_MARGIN of the plane or of fn0 = 0"""
    n = len(st["root_states"])
    cfg = S.step_cfg(n, asset)
    rs = st["root_states"].copy()
    z0 = rs[:, :, 2].copy()
    todo = ~ground_kept(st, asset, cfg)
    for k in (1, -1, 2, -2, 3, -3):
        if not todo.any():
            break
        rs[todo, :, 2] = z0[todo] + np.float32(k * NUDGE)
        ok = ground_kept(dict(st, root_states=rs), asset, cfg)
        rs[todo & ~ok, :, 2] = z0[todo & ~ok]
        todo &= ~ok
    return dict(st, root_states=rs)


_STATES = {}


def case_states(scenario, asset, n, task="bez_kick", fixed=False):
    """the states of a scenario, generated once per process: root_states (n, actors, 13), dof_state (n, 18, 2), actions (n, 18), fp32;
    `late`: and `first`, the state the call is made from"""
    key = (scenario, asset, n, task, fixed)
    if key in _STATES:
        return _STATES[key]
    if scenario in ("flight", "late"):
        st = flight_states(n, asset, fixed=fixed)
        if scenario == "late":
            st = dict(st, first=flight_states(n, asset, seed=22))
    elif scenario == "stance":
        st = dict(_off_the_ground_edges(B.kick_stance_states(n, asset, 3), asset), actions=S.actions(n, 2))
    else:
        assert scenario == "lying", scenario
        st = dict(_off_the_ground_edges(G.lying_states(n, asset), asset), actions=S.actions(n, 2))
    if task != "bez_kick":   # no ball actor
        st = {k: (v[:, :1].copy() if k == "root_states" else v) for k, v in st.items()}
        if "first" in st:
            st["first"] = dict(st["first"], root_states=st["first"]["root_states"][:, :1].copy())
    _STATES[key] = st
    return st


def body_frames(asset, task, st):
    """(rotation (n, rows, 3, 3), origin in env coordinates (n, rows, 3)) of every body row of the state st, the ball's included: an
    independent forward-kinematics pass (generalized_forces_numpy.body_velocities)"""
    root = st["root_states"][:, 0].astype(np.float64)
    _, rot, pos = GF.body_velocities(GF.model_of(asset), root, st["dof_state"].astype(np.float64))
    pos = pos + root[:, None, 0:3]
    if task == "bez_kick":
        ball = st["root_states"][:, 1].astype(np.float64)
        rot = np.concatenate([rot, B.quat_to_mat(ball[:, 3:7])[:, None]], 1)
        pos = np.concatenate([pos, ball[:, None, 0:3]], 1)
    return rot, pos


# ---------------------------------------------------------------------------------------------------------------- loads
def solo_cells(n, nbe):
    """(body, mode) of every env of the solo pattern"""
    e = np.arange(n)
    return e % nbe, (e // nbe) % len(MODES)


def _unit(rng, shape):
    v = rng.normal(size=shape)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _call(T, frames, keep, F, Tq, P, space, points, torque):
    """one call [forces, torques or None, positions or None, space] on the rows `keep` (n, rows); the position rows of unloaded bodies
    stay filled: the call must not read them"""
    rot, pos = frames
    com = np.concatenate([T.com, np.zeros((T.nbe - T.nb, 3))], 0)
    X = None
    if points:
        X = com[None] + P if space == LOCAL else pos + np.einsum("nbij,bj->nbi", rot, com) + P
    return [np.where(keep[..., None], F, 0.0), np.where(keep[..., None], Tq, 0.0) if torque else None, X, space]


_MINV = {}


def _minv(key, asset, st, mass_scale, armature):
    """(n, 24, 24) fp64 inverse mass matrices of the states, u = [root_lin, root_ang, qd]"""
    if key not in _MINV:
        M = FD.M_batch(GF.model_of(asset), st["root_states"][:, 0].astype(np.float64), st["dof_state"].astype(np.float64), mass_scale, armature)
        _MINV[key] = np.linalg.inv(M)
    return _MINV[key]


def _scale(calls, T, asset, st, cfg, rng, level, mass_scale, minv_key):
    """the magnitudes of the module docstring, in place; calls hold fp64 unit draws"""
    model = GF.model_of(asset)
    root, dof = st["root_states"][:, 0].astype(np.float64), st["dof_state"].astype(np.float64)
    n, nb, dt = len(root), T.nb, float(cfg.dt)
    Minv = _minv(minv_key, asset, st, mass_scale, float(cfg.armature))
    mb, Ib = float(B.model()["ball"]["mass"]), float(B.model()["ball"]["inertia"])

    def rate(rows, F, Tq, X, space):
        Q = GF.gf_ref(model, root[rows], dof[rows], None if F is None else F[rows], None if Tq is None else Tq[rows],
                      None if X is None else X[rows], space)
        return np.abs(dt * np.einsum("nij,nj->ni", Minv[rows], Q)[:, 6:]).max(1)
    for F, Tq, X, space in calls:
        for A in (F, Tq):
            if A is None:
                continue
            for b in range(nb):
                rows = np.flatnonzero((A[:, b] != 0).any(1))
                if len(rows):
                    one = np.zeros_like(A); one[rows, b] = A[rows, b]
                    A[rows, b] /= rate(rows, one if A is F else None, one if A is Tq else None, X, space)[:, None]
        if T.ball:
            F[:, nb] *= mb / dt
            if Tq is not None:
                Tq[:, nb] *= Ib / dt
    total = sum(GF.gf_ref(model, root, dof, F, Tq, X, space) for F, Tq, X, space in calls)
    a = np.abs(dt * np.einsum("nij,nj->ni", Minv, total)[:, 6:]).max(1)
    want = rng.uniform(*EASY, n) * (rng.uniform(*HARD, n) if level == "hard" else 1.0)
    ball = rng.uniform(*EASY, n) * (rng.uniform(*HARD, n) if level == "hard" else 1.0)
    s = np.where(a > 0, want / np.where(a > 0, a, 1.0), 0.0)
    for F, Tq, X, space in calls:
        for A in (F, Tq):
            if A is not None:
                A[:, :nb] *= s[:, None, None]
                A[:, nb:] *= ball[:, None, None]


def loads(pattern, asset, task, states, seed, level="easy", cfg=None, mass_scale=None, minv_key=None):
    """-> (calls, aimed): the calls [F, T, X or None, space] of a pattern, fp32 (n, rows, 3), for the state `states` (the state the call
    is made from), and the rows they load, (n, rows) bool"""
    T = tables(asset, task)
    n, nbe = len(states["root_states"]), T.nbe
    rng = np.random.default_rng(seed)
    frames = body_frames(asset, task, states)
    draw = lambda: (_unit(rng, (n, nbe, 3)), _unit(rng, (n, nbe, 3)), rng.uniform(-REACH, REACH, (n, nbe, 3)))
    if pattern in ("solo", "sparse"):
        body, mode = solo_cells(n, nbe)
        on = np.ones(n, bool)
        if pattern == "sparse":
            on[:] = False; on[list(S.NEIGHBOUR_ENVS)] = True
        F, Tq, P = draw()
        calls = []
        for m, name in enumerate(MODES):
            keep = np.zeros((n, nbe), bool)
            rows = np.flatnonzero(on & (mode == m))
            keep[rows, body[rows]] = True
            calls.append(_call(T, frames, keep, F, Tq, P, LOCAL if name.startswith("local") else ENV, name.endswith("point"), name.endswith("centre")))
    elif pattern == "all":
        F, Tq, P = draw()
        calls = [_call(T, frames, np.ones((n, nbe), bool), F, Tq, P, ENV, True, True)]
    else:
        assert pattern == "stacked", pattern
        always = [T.names.index(x) for x in ALWAYS]
        calls = []
        for space, points in ((ENV, False), (LOCAL, True), (ENV, True)):
            F, Tq, P = draw()
            keep = rng.uniform(size=(n, nbe)) < 1.0 / 3.0
            keep[:, always] = True
            calls.append(_call(T, frames, keep, F, Tq, P, space, points, True))
    _scale(calls, T, asset, states, cfg, rng, level, mass_scale, minv_key)
    aimed = np.zeros((n, nbe), bool)
    for c in calls:
        aimed |= (c[0] != 0).any(2)
        if c[1] is not None:
            aimed |= (c[1] != 0).any(2)
    return [[None if a is None else a.astype(np.float32) for a in c[:3]] + [c[3]] for c in calls], aimed


# ---------------------------------------------------------------------------------------------------------------- the oracle's side of a case
SLIPS = ("force_5pc", "point_2mm", "frame_frozen", "local_as_env", "fixed_body_offset_dropped", "ball_point_fixed_in_world",
         "second_call_overwrites", "acts_twice", "rows_shifted", "predictor_blind")
# the case each slip is looked for in: reference(**kw)
SLIP_CASES = {"force_5pc": dict(), "point_2mm": dict(), "frame_frozen": dict(substeps=4), "local_as_env": dict(),
              "fixed_body_offset_dropped": dict(asset="cleats"), "ball_point_fixed_in_world": dict(substeps=4),
              "second_call_overwrites": dict(pattern="stacked"), "acts_twice": dict(steps=2), "rows_shifted": dict(),
              "predictor_blind": dict(level="hard")}


def slipped_calls(calls, slip):
    """the calls as a wrong implementation of the call would take them (the slips that need no hook in the oracle)"""
    if slip == "force_5pc":
        return [[c[0] * np.float32(1.05)] + c[1:] for c in calls]
    if slip == "second_call_overwrites":
        return calls[-1:]
    if slip == "rows_shifted":   # body row b read as b + 1
        return [[None if a is None else np.roll(a, -1, axis=1) for a in c[:3]] + [c[3]] for c in calls]
    return calls


def run(ref, precision, loaded, slip=None):
    """one oracle through the case: (outputs, decision words (n, steps x substeps, 18), decisions of every step)"""
    from oracle.bez_oracle import Oracle
    o = Oracle(ref.cfg(), precision=precision)
    if slip in Oracle.EXT_SLIPS:
        o.set_ext_slip(slip)
    inject(o, ref.states.get("first", ref.states), ref.params)
    if loaded:
        for F, Tq, X, space in slipped_calls(ref.calls, slip):
            o.apply_body_forces(F, Tq, X, space)
    if "first" in ref.states:
        inject(o, ref.states, ref.params)
    decisions = []
    for _ in range(ref.steps):
        o.step(ref.actions)
        decisions.append(o.joint_decisions())
    return outputs(o, ref.n), np.concatenate([d["word"] for d in decisions], 1), decisions


def reference(scenario="flight", pattern="solo", level="easy", asset="default", n=N, substeps=2, dr=False, flags=0, task="bez_kick", steps=1):
    """step_terms.reference of a wrench case, with this module's own runs: one control step (steps=2: two, the second without a call) of
    the fp64 oracle and of its fp32 build, loaded and unloaded -- states, per-env parameters, actions, calls, aimed rows, the four
    outputs, the decision words, kept, the responses d64 / d32 = loaded - unloaded."""
    flags &= ~abi.FLAG_DOF_FORCE    # the oracle records its actuators anyway; the sims of the GPU file set the flag themselves

    def cfg():
        c = S.step_cfg(n, asset, gravity=scenario in GRAVITY, substeps=substeps, flags=flags)
        c.task = abi.TASK_IDS[task]
        return c

    def build(ref):
        ref.cfg = cfg
        fixed = bool(flags & FIXED_BASE)
        ref.states = case_states(scenario, asset, n, task, fixed)
        ref.actions = ref.states["actions"]
        ref.params = None
        if dr:
            ref.params = dict(S.dr_params(n, 8))
            ref.params[abi.PARAM_MASS_SCALE] = np.random.default_rng(9).uniform(0.8, 1.2, (n, 19)).astype(np.float32)
        scale = None if not dr else ref.params[abi.PARAM_MASS_SCALE].astype(np.float64)
        at = ref.states.get("first", ref.states)
        ref.calls, ref.aimed = loads(pattern, asset, task, at, 31, level, cfg(), scale, (scenario, asset, n, task, fixed, dr))
        ref.body, ref.mode = solo_cells(n, ref.tables.nbe)
        ref.out64, ref.words64, dec_l = run(ref, "f64", True)
        ref.unl64, ref.words64_unl, dec_u = run(ref, "f64", False)
        ref.out32, ref.words32, _ = run(ref, "f32", True)
        ref.unl32, _, _ = run(ref, "f32", False)
        ref.kept = np.ones(n, bool)
        for d in dec_l + dec_u:
            ref.kept &= J.kept(d)
        ref.joints_kept = ref.kept.copy()
        if scenario in GRAVITY:
            from oracle.bez_oracle import Oracle
            o = Oracle(cfg())
            inject(o, ref.states, ref.params)
            rb = o.rigid_body_states.reshape(n, -1, 13)
            ref.kept &= G.kept(G.terms(ref.states, asset, rb, cfg()))
            if scenario == "stance":
                ref.kept &= B.kept(B.depths(rb, ref.states["root_states"][:, 1, 0:3], asset))
        ref.err32 = S.env_errors(ref.out32, ref.out64)
        ref.d64 = {q: ref.out64[q] - ref.unl64[q] for q in RESPONSE}
        ref.d32 = {q: ref.out32[q] - ref.unl32[q] for q in RESPONSE}
        ref.rerr32 = {q: np.abs(ref.d32[q] - ref.d64[q]).max(1) for q in RESPONSE}
    return S.reference(("wrench", scenario, pattern, level, asset, n, substeps, dr, flags, task, steps), build,
                       scenario=scenario, pattern=pattern, level=level, asset=asset, n=n, substeps=substeps, dr=dr, flags=flags, task=task,
                       steps=steps, tables=tables(asset, task))


def new_bits(ref):
    """(n,) bool: envs with a saturation or lock bit, in some substep and joint, that the unloaded twin does not have (fp64)"""
    return ((ref.words64 & J.STATUS_BITS) & ~(ref.words64_unl & J.STATUS_BITS)).any((1, 2))


def response_bars(ref):
    """quantity of RESPONSE -> (bar, the fp32 build's worst): 3 x the fp32 build's worst |d32 - d64| over the kept envs outside the
    OUTLIER_BUDGET envs the kernel is allowed, + 2 ulp32 of the largest |fp64 output| -- measured on the oracle's two builds, never on
    a kernel"""
    out = {}
    for q in RESPONSE:
        worst = float(np.sort(ref.rerr32[q][ref.kept])[-1 - S.OUTLIER_BUDGET])
        out[q] = (3.0 * worst + 2.0 * float(np.spacing(np.float32(np.abs(ref.out64[q][ref.kept]).max()))), worst)
    return out


def response_errors(ref, out, out_unloaded):
    """quantity of RESPONSE -> (n,) the largest |(out - out_unloaded) - d64| of every env (inf for a non-finite env)"""
    res = {}
    for q in RESPONSE:
        d = out[q] - out_unloaded[q]
        res[q] = np.where(np.isfinite(d).all(1), np.abs(d - ref.d64[q]).max(1), np.inf)
    return res


def compare(case, ref, out, out_unloaded, label, report=None, p99=True):
    """One stepped simulator against the fp64 oracle.
    (a) step_terms.compare: every kept env inside case_bars with EnvOutliers' default budget, reset flags equal outside the outliers,
        per quantity the p99 of |got - f64| at most 2.5 x the fp32 build's + 1e-6 (p99=False: printed only).
    (b) the response out - out_unloaded (the same simulator stepped from the same state with nothing applied) against the oracle's,
        per quantity of RESPONSE: a loaded kept env beyond response_bars is an outlier of the SAME budget as (a)'s (the fp32 build's
        own worst is taken outside that budget, and a contact's friction kink is no more guarded by `kept` for the response than for
        the step); every (body, mode) cell of a solo case keeps more envs than the budget, so a wrench wrong for one body in one
        mode cannot hide in it.  Per loaded body row the worst error over its kept envs outside the outliers is reported.
    report: a function that receives (errors, outliers, bars, response errors, response bars, {body: {quantity: worst}}) before anything
    is asserted.  -> the mask of the outlier envs"""
    rbars = response_bars(ref)
    rerr = response_errors(ref, out, out_unloaded)
    beyond = ref.aimed.any(1) & np.any([~(rerr[q] <= rbars[q][0]) for q in RESPONSE], 0)

    def elements(bars, bad):
        bodies = {}
        for b in range(ref.tables.nbe):
            envs = ref.kept & ~bad & ref.aimed[:, b]
            if envs.any():
                bodies[b] = {q: float(rerr[q][envs].max()) for q in RESPONSE}
        for q in RESPONSE:
            print("%s %s response %-9s bar %.2e: fp32 build %.2e, here %.2e" % (case, label, q, rbars[q][0], rbars[q][1],
                                                                               max([v[q] for v in bodies.values()] or [0.0])))
        return (rerr, rbars, bodies), []
    return S.compare(case, ref, out, label, report=report, p99=p99, also_outliers=beyond, elements=elements)


def cells(ref):
    """(rows, 4) kept envs of every (body, mode) cell of a solo case"""
    out = np.zeros((ref.tables.nbe, len(MODES)), int)
    np.add.at(out, (ref.body[ref.kept], ref.mode[ref.kept]), 1)
    return out


def response_table(ref):
    """{quantity: (worst, p99)} of the fp32 build's response against fp64's over the kept envs (beside step_terms.error_table)"""
    k = ref.kept
    return {q: (float(ref.rerr32[q][k].max()), float(np.quantile(ref.rerr32[q][k], 0.99))) for q in RESPONSE}


def report_line(name, ref, err, outliers, bars, rerr, rbars, bodies):
    """one line of the report: step_terms.report_words with, before the raised bars, per response quantity the bar, worst / p99 of the
    kernel | of the fp32 build"""
    k = ref.kept
    words = S.report_words(name, 44, ref, err, outliers, bars)
    for q in RESPONSE:
        h, c = rerr[q][k], ref.rerr32[q][k]
        words.insert(-1, "d_%s=bar %.1e %.1e/%.1e|%.1e/%.1e" % (q, rbars[q][0], max([v[q] for v in bodies.values()] or [0.0]), np.quantile(h, 0.99),
                                                                c.max(), np.quantile(c, 0.99)))
    return "  ".join(words)


# every oracle case of tests/test_gpu_body_wrench.py: name -> reference(**kw)
CASES = {}
for _a in S.ASSETS:
    for _dr in (False, True):
        CASES["flight-solo-s2-%s %s" % ("dr" if _dr else "plain", _a)] = dict(asset=_a, dr=_dr)
for _s in (1, 3, 4):
    CASES["flight-solo-s%d-plain default" % _s] = dict(substeps=_s)
CASES["flight-solo-s4-plain cleats"] = dict(asset="cleats", substeps=4)
CASES["flight-solo-hard default"] = dict(level="hard")
for _sc in ("stance", "lying"):
    for _a in ("default", "cleats"):
        CASES["%s-solo %s" % (_sc, _a)] = dict(scenario=_sc, asset=_a)
for _p in ("all", "stacked"):
    for _a in S.ASSETS:
        CASES["flight-%s %s" % (_p, _a)] = dict(pattern=_p, asset=_a)
CASES["late-solo default"] = dict(scenario="late")
CASES["flight-solo walk default"] = dict(task="bez_walk")
CASES["flight-solo fixed-base default"] = dict(flags=FIXED_BASE)
CASES["flight-sparse200 default"] = dict(pattern="sparse", n=200)
SOLO = [k for k, v in CASES.items() if v.get("pattern", "solo") == "solo"]
HARD_CASES = [k for k, v in CASES.items() if v.get("level") == "hard"]


def planted(slip):
    """(ref, outputs, words): a case and the fp32 build's loaded outputs and decision words of the same case with one thing made wrong --
    on the oracle side only, no kernel is edited (the unloaded twin is ref.unl32).
      force_5pc                   every force x 1.05
      point_2mm                   every point of application 2 mm along x of its link's frame
      frame_frozen                the link frames of the first substep in every substep, 4 substeps
      local_as_env                LOCAL vectors left unrotated
      fixed_body_offset_dropped   BEZ_BODY_OFFSET of /camera and of the first cleat ignored (cleats asset)
      ball_point_fixed_in_world   the ball's point not turning with the ball, 4 substeps
      second_call_overwrites      `stacked` keeps only the last call
      acts_twice                  not dropped after the launch: two launches
      rows_shifted                body row b read as b + 1
      predictor_blind             the wrench propagated beside pA as the leg <-> leg wrenches are, unseen by the predictors; `hard`"""
    assert slip in SLIPS
    ref = reference(**SLIP_CASES[slip])
    out, words, _ = run(ref, "f32", True, slip)
    return ref, out, words
