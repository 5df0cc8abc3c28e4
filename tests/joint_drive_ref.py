"""The joint terms of the fused step, joint by joint: state generators that aim one joint per env at one branch of joint_terms /
joint_scalar (bez_kernels.h) -- beyond a limit, saturated, locked on the speed limit, across the friction floor --, the oracle's own
decision words and decision margins (oracle.bez_oracle.Oracle.joint_decisions), and the oracle's side, the comparison and the planted
slips of tests/test_joint_drive_cpu.py and tests/test_gpu_joint_drive.py (on the harness of tests/step_terms.py).

Per joint and substep the step decides (oracle: dynamics_x pass 2):
  below lo / above hi   q against the env's bounds: the implicit limit spring-damper limit_k, limit_d
  saturated + / -       the held-parent predictor tau_drive against +-effort: the drive is the effort and k_pd leaves the denominator
  locked + / -          the held-parent predictor v_pred against +-vel_limit: a prescribed-rate joint (g = 0, w = fix)
and, not a branch but a kink, the friction coefficient joint_friction / max(|qd|, jfric_veps).

Scenarios (`case_states`), all but the last in zero gravity with a floating base, the ball 3 m away, the legs LEG_CLEAR apart, every joint
LIMIT_MARGIN inside the limits and in the easy regime (target within EASY_TARGET of q, |qd| <= EASY_RATE) unless aimed:
  limits    env e aims joint e % 18 at regime (e // 18) % 3 of below lo by BEYOND, above hi by BEYOND, inside; its rate within +-LIMIT_RATE.
            Plain: the state lies beyond the model's limits.  dr: the posture stays inside them and the env's own PARAM_DOF_LOWER /
            PARAM_DOF_UPPER are moved inside the posture, every other bound of the env BOUND_SHIFT inside the model's.
  drive     env e aims joint e % 18 at regime (e // 18) % 4 of saturated +, saturated -, locked +, locked -
  friction  the aimed joint's |qd| log-uniform over a decade on each side of jfric_veps, both signs, its target on q
  pressed   tests/scenarios._pressed_state standing on the ground under gravity: six leg joints per env near the lock and saturated"""
import numpy as np

from bez_isaacgym_amd import abi
from tests import ball_contact_ref as B
from tests import step_terms as S
from tests.leg_contact_ref import pair_geometry, CLEAR

ND = 18
N = S.N
LIMIT_MARGIN = 0.03         # rad: the postures stay this far inside the joint limits
BEYOND = (0.01, 0.1)        # rad beyond the bound
BOUND_SHIFT = (0.005, 0.02)  # rad: the dr variant's non-aimed bounds lie this far inside the model's
LIMIT_RATE = 1.5            # rad/s: the aimed joint of `limits` moves toward or away from its bound at up to this
EASY_TARGET = 0.003        # rad: the easy drive leaves the rate below jfric_veps after a substep too
EASY_RATE = 0.05            # rad/s: below jfric_veps, so that no easy joint sits on the friction floor's kink
POSTURE = 0.3               # rad around the default pose
SAT_EXCESS = (1.1, 2.0)     # the saturated predictor exceeds the effort by 10 - 100 %
LOCK_RATE = (0.90, 1.00)    # share of vel_limit at which the locked regimes start
BALL_AWAY = 3.0             # m
LEG_CLEAR = CLEAR           # m: no leg pair closer than this at the start (a hip at its inner limit leaves under a millimetre)
BALL_DEPTH = 1e-3           # m: `pressed` has the parked ball this deep in the ground
REDRAW = 200                # candidate postures per env and round of _base's redraw
GRAVITY = ("pressed",)
BELOW, ABOVE, INSIDE = 0, 1, 2
SAT_POS, SAT_NEG, LOCK_POS, LOCK_NEG = 0, 1, 2, 3
REGIMES = {"limits": ("below_lo", "above_hi", "inside"), "drive": ("saturated+", "saturated-", "locked+", "locked-"),
           "friction": ("below_veps", "above_veps"), "pressed": ("pressed",)}
WORD_BELOW, WORD_ABOVE = 16, 32     # Oracle.JD_BELOW_LO / JD_ABOVE_HI
STATUS_BITS = 15                    # the four bits of BEZ_ACTUATOR_STATUS
# what the aimed joint's decision word must show in each regime: (mask, value)
SHOWS = {"limits": ((WORD_BELOW | WORD_ABOVE, WORD_BELOW), (WORD_BELOW | WORD_ABOVE, WORD_ABOVE), (WORD_BELOW | WORD_ABOVE, 0)),
         "drive": ((abi.ACTUATOR_SATURATED, abi.ACTUATOR_SATURATED_POS), (abi.ACTUATOR_SATURATED, abi.ACTUATOR_SATURATED_NEG),
                   (abi.ACTUATOR_LOCKED, abi.ACTUATOR_LOCKED_POS), (abi.ACTUATOR_LOCKED, abi.ACTUATOR_LOCKED_NEG))}

# The knife-edge margins of `kept` (DESIGN.md 6 "knife edges"), one per decision quantity.  *_MEASURED: the smallest margin at which the
# oracle's fp32 build takes the fp64 build's decision word in every kept env of every case of CASES (measure_margins;
# tests/test_joint_drive_cpu.py re-measures and prints them); the margin itself is twice that, because the kernels round differently
# from the fp32 build.
TORQUE_MEASURED = 3.25e-4     # N m     tau_drive against +-effort
RATE_MEASURED = 2.33e-4       # rad/s   v_pred against +-vel_limit
ANGLE_MEASURED = 3.52e-7      # rad     q against lo and hi
FLOOR_MEASURED = 3.35e-6      # rad/s   |qd| against jfric_veps
TORQUE_MARGIN, RATE_MARGIN, ANGLE_MARGIN, FLOOR_MARGIN = 2 * TORQUE_MEASURED, 2 * RATE_MEASURED, 2 * ANGLE_MEASURED, 2 * FLOOR_MEASURED
MARGIN_OF = {"m_tau": "torque", "m_vel": "rate", "m_fric": "floor", "m_lo": "angle", "m_hi": "angle"}
KINDS = ("torque", "rate", "angle", "floor")


def margins():
    return {"torque": TORQUE_MARGIN, "rate": RATE_MARGIN, "angle": ANGLE_MARGIN, "floor": FLOOR_MARGIN}


def model_limits():
    m = B.model()
    return np.asarray(m["dof_lower"], np.float32).astype(np.float64), np.asarray(m["dof_upper"], np.float32).astype(np.float64)


def targets_of(act):
    """the position targets the step forms from an action row, in its own fp32 arithmetic (oracle: env_pre_physics)"""
    m = B.model()
    a = np.clip(np.asarray(act, np.float32), np.float32(-3.9), np.float32(3.9))
    a[:, :2] = 0.0
    t = a + np.asarray(m["dof_default"], np.float32)
    return np.clip(t, np.asarray(m["dof_lower"], np.float32), np.asarray(m["dof_upper"], np.float32))


# ---------------------------------------------------------------------------------------------------------------- generators
def _base(n, asset, rng, fix=None):
    """root, ball and an easy posture: (rs (n, 2, 13), q, qd, target (n, 18)); fix(q, rng) edits the posture before the legs are checked,
    and is applied again to every redrawn env"""
    m = B.model()
    lo, hi = model_limits()
    dflt = np.asarray(m["dof_default"], np.float64)
    rs = np.zeros((n, 2, 13))
    quat = rng.normal(size=(n, 4)); quat /= np.linalg.norm(quat, axis=1, keepdims=True)
    rs[:, 0, 2] = 1.0
    rs[:, 0, 3:7] = quat
    rs[:, 0, 7:10] = rng.uniform(-0.3, 0.3, (n, 3))
    rs[:, 0, 10:13] = rng.uniform(-1.0, 1.0, (n, 3))
    rs[:, 1, 0:3] = rs[:, 0, 0:3] + (0.0, BALL_AWAY, 0.0)
    rs[:, 1, 6] = 1.0

    def draw(k, wide):
        if wide:
            q = rng.uniform(lo + LIMIT_MARGIN, hi - LIMIT_MARGIN, (k, ND))
        else:
            q = np.clip(dflt + rng.uniform(-POSTURE, POSTURE, (k, ND)), lo + LIMIT_MARGIN, hi - LIMIT_MARGIN)
        q[:, :2] = rng.uniform(-EASY_TARGET, EASY_TARGET, (k, 2))   # the head joints' targets are their defaults: the easy regime is next to them
        return q

    def clear(rows, q):
        gap, _, _ = pair_geometry(quat[rows].astype(np.float32), q.astype(np.float32), asset)
        return gap.min(1) >= LEG_CLEAR
    q = draw(n, False)
    if fix is not None:
        fix(q, np.arange(n))
    bad = np.flatnonzero(~clear(np.arange(n), q))
    # Redrawn, REDRAW candidates per env at a time: around the default pose first, then anywhere inside the limits (a hip at its inner
    # limit clears the other leg in under 1 % of the postures, and only with both legs far from the default pose)
    for it in range(14):
        if not len(bad):
            break
        wide = it >= 2
        m = REDRAW if wide else 8
        rows = np.repeat(bad, m)
        cand = draw(len(rows), wide)
        if fix is not None:
            fix(cand, rows, local=True)
        ok = clear(rows, cand).reshape(len(bad), m)
        first = ok.argmax(1)
        got = ok.any(1)
        q[bad[got]] = cand.reshape(len(bad), m, ND)[np.flatnonzero(got), first[got]]
        bad = bad[~got]
    assert not len(bad), len(bad)
    qd = rng.uniform(-EASY_RATE, EASY_RATE, (n, ND))
    target = np.clip(q + rng.uniform(-EASY_TARGET, EASY_TARGET, (n, ND)), lo, hi)
    target[:, :2] = 0.0
    return rs, q, qd, target


def _finish(rs, q, qd, target, **more):
    dflt = np.asarray(B.model()["dof_default"], np.float64)
    ds = np.stack([q, qd], -1)
    act = (target - dflt).astype(np.float32)
    return dict(root_states=rs.astype(np.float32), dof_state=ds.astype(np.float32), actions=act, **more)


def limits_states(n, asset, dr, seed=11):
    rng = np.random.default_rng(seed)
    lo, hi = model_limits()
    env = np.arange(n)
    aim, regime = env % ND, (env // ND) % 3
    beyond = rng.uniform(*BEYOND, n)

    def fix(q, rows, local=False):
        if dr:
            return
        at = np.arange(len(rows)) if local else rows
        j, r = aim[rows], regime[rows]
        q[at, j] = np.where(r == BELOW, lo[j] - beyond[rows], np.where(r == ABOVE, hi[j] + beyond[rows], q[at, j]))
    rs, q, qd, target = _base(n, asset, rng, fix)
    qd[env, aim] = np.where(regime == INSIDE, qd[env, aim], rng.uniform(-LIMIT_RATE, LIMIT_RATE, n))
    target = np.clip(target, lo, hi)
    target[:, :2] = 0.0
    params = None
    if dr:
        elo = np.tile(lo, (n, 1)) + rng.uniform(*BOUND_SHIFT, (n, ND))
        ehi = np.tile(hi, (n, 1)) - rng.uniform(*BOUND_SHIFT, (n, ND))
        q32 = q.astype(np.float32).astype(np.float64)
        elo[env, aim] = np.where(regime == BELOW, q32[env, aim] + beyond, elo[env, aim])
        ehi[env, aim] = np.where(regime == ABOVE, q32[env, aim] - beyond, ehi[env, aim])
        params = dict(S.dr_params(n, seed + 1))
        params[abi.PARAM_DOF_LOWER] = elo.astype(np.float32)
        params[abi.PARAM_DOF_UPPER] = ehi.astype(np.float32)
    return _finish(rs, q, qd, target, aim=aim, regime=regime, params=params)


def _joint_inertia(asset):
    """(18,) a nominal inertia about each joint axis of everything outboard of it, in the default pose, from the model JSON (point
    masses at the links' centres of mass plus the links' own inertias about the axis are not needed to 10 %: the generators only
    size the target offsets with it, and the CPU test checks the regimes the oracle really takes)"""
    links = B.asset_links(asset)
    dflt = np.asarray(B.model()["dof_default"], np.float64)[None]
    E, r = B.link_frames(asset, np.zeros((1, 3)), np.array([[0.0, 0.0, 0.0, 1.0]]), dflt)
    nl = len(links)
    parent = [links[i]["parent"] for i in range(nl)]
    out = np.zeros(ND)
    for l in range(1, nl):
        axis = E[0, parent[l]] @ np.asarray(links[l]["axis"], np.float64)
        for k in range(l, nl):
            a = k
            while a > l:
                a = parent[a]
            if a != l:
                continue
            c = r[0, k] + E[0, k] @ np.asarray(links[k]["com"], np.float64) - r[0, l]
            perp = c - axis * (c @ axis)
            out[l - 1] += float(links[k]["mass"]) * (perp @ perp)
    return out


def _predicted_gain(cfg, asset, joint, rate, kp_scale, kd_scale):
    """d tau_drive / d tau_pd0 of the held-parent predictor, (J + k_f) / (J + k_pd + k_f), per env for its aimed joint: the nominal J,
    the env's gain scales and the friction coefficient at the joint's rate"""
    h = float(cfg.dt) / int(cfg.substeps)
    J = _joint_inertia(asset)[joint] + float(cfg.armature)
    k_pd = h * h * float(cfg.kp) * kp_scale + h * float(cfg.kd) * kd_scale
    k_f = h * float(cfg.joint_friction) / np.maximum(np.abs(rate), float(cfg.jfric_veps))
    return (J + k_f) / (J + k_pd + k_f)


def drive_states(n, asset, cfg, dr, seed=12, only=None):
    """The aimed joint's target is the bound ahead of it (0 for the head joints, whose targets are their defaults) and q so far behind
    that the explicit PD torque kp (target - q - h qd) - kd qd times _predicted_gain -- the held-parent predictor tau_drive up to the
    bias forces -- exceeds the effort by SAT_EXCESS, or as far behind as the joint's range allows.  saturated +-: from rest; locked +-:
    from LOCK_RATE x vel_limit, so that the saturated drive carries v_pred over the limit.  kp, kd, the effort, the speed limit and
    the gain come from cfg and, with dr, from the env's Kp / Kd scales."""
    rng = np.random.default_rng(seed)
    lo, hi = model_limits()
    env = np.arange(n)
    aim, regime = env % ND, (env // ND) % 4
    easy = np.zeros(n, bool)
    if only is not None:
        easy[:] = True; easy[np.asarray(only, int)] = False
    params = dict(S.dr_params(n, seed + 1)) if dr else None
    kps = params[abi.PARAM_KP_SCALE][env, aim].astype(np.float64) if dr else np.ones(n)
    kds = params[abi.PARAM_KD_SCALE][env, aim].astype(np.float64) if dr else np.ones(n)
    sign = np.where((regime == SAT_POS) | (regime == LOCK_POS), 1.0, -1.0)
    lock = regime >= LOCK_POS
    kp, kd, eff, vl = float(cfg.kp) * kps, float(cfg.kd) * kds, float(cfg.effort), float(cfg.vel_limit)
    h = float(cfg.dt) / int(cfg.substeps)
    speed = np.where(lock, rng.uniform(*LOCK_RATE, n) * vl, 0.0)
    want = rng.uniform(*SAT_EXCESS, n) * eff / _predicted_gain(cfg, asset, aim, speed, kps, kds)
    delta = (want + kd * speed) / kp + h * speed
    room = np.where(aim < 2, np.minimum(-lo[aim], hi[aim]), (hi - lo)[aim]) - LIMIT_MARGIN
    delta = np.minimum(delta, room)

    def fix(q, rows, local=False):
        at = (np.arange(len(rows)) if local else rows)[~easy[rows]]
        rows = rows[~easy[rows]]
        j, s = aim[rows], sign[rows]
        tgt = np.where(j < 2, 0.0, np.where(s > 0, hi[j], lo[j]))
        q[at, j] = tgt - s * delta[rows]
    rs, q, qd, target = _base(n, asset, rng, fix)
    a = ~easy
    qd[env[a], aim[a]] = (sign * speed)[a]
    target[env[a], aim[a]] = np.where(aim[a] < 2, 0.0, np.where(sign[a] > 0, hi[aim[a]], lo[aim[a]]))
    return _finish(rs, q, qd, target, aim=np.where(easy, -1, aim), regime=regime, params=params)


def friction_states(n, asset, cfg, seed=13):
    rng = np.random.default_rng(seed)
    env = np.arange(n)
    aim = env % ND
    rs, q, qd, target = _base(n, asset, rng)
    veps = float(cfg.jfric_veps)
    speed = veps * 10.0 ** rng.uniform(-1.0, 1.0, n)
    qd[env, aim] = rng.choice([-1.0, 1.0], n) * speed
    q[:, :2] = np.where((aim[:, None] == np.arange(2)[None]), 0.0, q[:, :2])   # an aimed head joint sits on its target, 0
    target[env, aim] = q.astype(np.float32)[env, aim]
    return _finish(rs, q, qd, target, aim=aim, regime=(speed > veps).astype(int), params=None)


PRESSED_FAST = (6, 7, 8, 14, 15, 16)


def pressed_states(n, asset, seed=14):
    """tests/scenarios._pressed_state with the hip rolls at the default pose (legs apart), upright at the reset height on the ground,
    the torso's twist at a tenth (tests/test_gpu_dof_force.py test_internal_consistency_on_the_ground_with_a_push)"""
    from tests.scenarios import _pressed_state
    rng = np.random.default_rng(seed)
    m = B.model()
    dflt = np.asarray(m["dof_default"], float)
    rs = np.zeros((n, 2, 13)); q = np.zeros((n, ND)); qd = np.zeros((n, ND)); target = np.zeros((n, ND))
    for e in range(n):
        q[e], qd[e], target[e], v0, _, _, _ = _pressed_state(m, rng)
        q[e, 5] = dflt[5]; q[e, 13] = dflt[13]; target[e, 5] = dflt[5]; target[e, 13] = dflt[13]
        rs[e, 0, 7:10] = 0.1 * v0[3:]; rs[e, 0, 10:13] = 0.1 * v0[:3]
    rs[:, 0, 0:3] = (0.0, 0.0, 0.34); rs[:, 0, 6] = 1.0
    rs[:, 1, 0:3] = B.PARKED; rs[:, 1, 6] = 1.0
    rs[:, 1, 2] = B.ball_radius() - BALL_DEPTH   # resting in the ground, off the knife edge of touching it
    return _finish(rs, q, qd, target, aim=np.full(n, -1), regime=np.zeros(n, int), params=None)


_STATES = {}


def case_states(scenario, asset, n, dr, cfg):
    """the states of a case, generated once per process (the planted slips step from the same states)"""
    key = (scenario, asset, n, dr)
    if key not in _STATES:
        _STATES[key] = _case_states(scenario, asset, n, dr, cfg)
    return _STATES[key]


def _case_states(scenario, asset, n, dr, cfg):
    if scenario == "limits":
        return limits_states(n, asset, dr)
    if scenario == "drive":
        return drive_states(n, asset, cfg, dr)
    if scenario == "drive_none":     # the drive states with nobody aimed
        return drive_states(n, asset, cfg, dr, only=())
    if scenario == "drive_sparse":   # drive_none with the envs NEIGHBOUR_ENVS taken from the drive states: the envs are independent
        full, none = case_states("drive", asset, n, dr, cfg), case_states("drive_none", asset, n, dr, cfg)
        rows = list(S.NEIGHBOUR_ENVS)
        out = {k: (None if v is None else v.copy()) for k, v in none.items() if k != "params"}
        for k in ("root_states", "dof_state", "actions", "aim"):
            out[k][rows] = full[k][rows]
        assert not dr
        return dict(out, params=None)
    if scenario == "friction":
        return friction_states(n, asset, cfg)
    assert scenario == "pressed", scenario
    return pressed_states(n, asset)


def family(scenario):
    return scenario.split("_")[0]


# ---------------------------------------------------------------------------------------------------------------- kept
def kept(m, marg=None):
    """envs in which every decision quantity of every joint stays at least its margin from its boundary in every substep.
    m: Oracle.joint_decisions() of the fp64 oracle; marg: {kind of KINDS: margin} (default: the module's constants)"""
    marg = margins() if marg is None else marg
    ok = np.ones(len(m["word"]), bool)
    for col, kind in MARGIN_OF.items():
        ok &= (m[col] >= marg[kind]).all((1, 2))
    return ok


def measure_margins(refs):
    """{kind of KINDS: margin}: the smallest margins at which the fp32 build's decision words equal the fp64 build's in every kept
    env of every ref.  An env whose words differ is charged to the decision that differs first (the earliest substep; there the differing
    decision nearest its boundary): the later ones follow from it.  A differing bit belongs to m_tau (saturated), m_vel (locked), m_lo,
    m_hi.  The generated states are too few next to the boundaries for that alone to say much, so each margin is also at least the
    largest difference between the two builds' distances of that kind in the envs whose words agree."""
    need = dict.fromkeys(KINDS, 0.0)
    bit_col = ((abi.ACTUATOR_SATURATED, "m_tau"), (abi.ACTUATOR_LOCKED, "m_vel"), (WORD_BELOW, "m_lo"), (WORD_ABOVE, "m_hi"))
    for ref in refs:
        diff = ref.words64 ^ ref.words32
        for e in np.flatnonzero(diff.any((1, 2))):
            s = int(np.flatnonzero(diff[e].any(1))[0])
            best = None
            for bits, col in bit_col:
                j = np.flatnonzero(diff[e, s] & bits)
                if len(j):
                    v = float(ref.decisions[col][e, s, j].min())
                    if best is None or v < best[0]:
                        best = (v, MARGIN_OF[col])
            need[best[1]] = max(need[best[1]], best[0])
        # and where the words agree, how far the fp32 build's decision quantities are from the fp64 build's: a decision nearer its
        # boundary than that is one the fp32 build may take the other way, whether or not a generated state happens to lie there
        same = ~diff.any((1, 2))
        for col, kind in MARGIN_OF.items():
            need[kind] = max(need[kind], float(np.abs(ref.decisions32[col][same] - ref.decisions[col][same]).max()))
    return need


# ---------------------------------------------------------------------------------------------------------------- the oracle's side of a case
def reference(scenario, asset, n, substeps=2, dr=False, flags=0, wrong=None, tag=None):
    """step_terms.reference of a joint case: states, per-env parameters, actions, both outputs, both builds' decision words
    (n, substeps, 18), the fp64 build's decisions with their margins, kept, aim (the aimed joint, -1: none) and aimed (n, 18), both
    actuator records.
    wrong / tag: a planted slip -- wrong(cfg, params) edits the oracle's config and parameters, the states stay the scenario's."""
    flags &= ~abi.FLAG_DOF_FORCE    # the oracle records its actuators anyway; the sims of the GPU file set the flag themselves

    def build(ref):
        ref.cfg = lambda: S.step_cfg(n, asset, gravity=family(scenario) in GRAVITY, substeps=substeps, flags=flags)
        ref.states = case_states(scenario, asset, n, dr, ref.cfg())
        ref.aim, ref.regime = ref.states["aim"], ref.states["regime"]
        ref.aimed = np.zeros((n, ND), bool)
        if family(scenario) == "pressed":
            ref.aimed[:, list(PRESSED_FAST)] = True
        else:
            ref.aimed[np.flatnonzero(ref.aim >= 0), ref.aim[ref.aim >= 0]] = True
        ref.params = ref.states["params"]
        if dr and ref.params is None:
            ref.params = dict(S.dr_params(n, 8))
        ref.actions = ref.states["actions"]
        ocfg, oparams = ref.cfg(), ref.params
        if wrong is not None:
            oparams = wrong(ocfg, None if oparams is None else dict(oparams))
        o64, o32 = S.oracle_pair(ref, ocfg, oparams)
        ref.ground = np.ones(n, bool)
        if family(scenario) in GRAVITY:
            from tests import ground_contact_ref as G
            ref.ground = G.kept(G.terms(ref.states, asset, o64.rigid_body_states.reshape(n, -1, 13), ref.cfg()))
        S.step_pair(ref, o64, o32)
        ref.decisions, ref.decisions32 = o64.joint_decisions(), o32.joint_decisions()
        ref.words64, ref.words32 = ref.decisions["word"], ref.decisions32["word"]
        ref.kept = kept(ref.decisions) & ref.ground
        ref.act64, ref.act32 = o64.actuators(), o32.actuators()
    return S.reference(("joint", scenario, asset, n, substeps, dr, flags, tag), build,
                       scenario=scenario, asset=asset, n=n, substeps=substeps, dr=dr, flags=flags)


ASSETS = tuple(S.ASSETS)
# every oracle case of tests/test_gpu_joint_drive.py: (scenario, asset, n, substeps, dr)
CASES = ([(s, a, N, 2, dr) for s in ("limits", "drive", "friction") for a in ASSETS for dr in (False, True)]
         + [("pressed", "default", N, k, False) for k in (1, 2, 3, 4)]
         + [(s, "default", 200, 2, False) for s in ("drive_sparse", "drive_none")])


def case_name(scenario, asset, n, substeps, dr):
    return "%s%s-s%d-%s %s" % (scenario, "" if n == N else str(n), substeps, "dr" if dr else "plain", asset)


def regime_counts(ref):
    """{regime name: (kept envs aimed at it, those whose aimed joint's fp64 decision word shows it in the first substep)}"""
    fam = family(ref.scenario)
    out = {}
    for r, name in enumerate(REGIMES[fam]):
        envs = np.flatnonzero(ref.kept & (ref.aim >= 0) & (ref.regime == r))
        if fam == "pressed":   # every env; shown: some joint locked and some joint saturated in some substep
            envs = np.flatnonzero(ref.kept)
            w = ref.words64[envs]
            shown = int((((w & abi.ACTUATOR_LOCKED) != 0).any((1, 2)) & ((w & abi.ACTUATOR_SATURATED) != 0).any((1, 2))).sum())
        elif fam in SHOWS:
            mask, value = SHOWS[fam][r]
            shown = int(((ref.words64[envs, 0, ref.aim[envs]] & mask) == value).sum())
        else:
            shown = len(envs)
        out[name] = (len(envs), shown)
    return out


def compare(case, ref, out, label, report=None, p99=True):
    """step_terms.compare, and per aimed joint the worst q and qd error of that joint in ALL its kept envs -- no outlier budget -- within
    the q / qd bars.  report receives {joint: (q worst, qd worst)} as its fourth argument."""
    def elements(bars, bad):
        joints = {}
        for j in range(ND):
            envs = ref.kept & ref.aimed[:, j]
            if envs.any():
                joints[j] = tuple(float(np.abs(out[x][envs, j] - ref.out64[x][envs, j]).max()) for x in ("q", "qd"))
        return (joints,), [("joint %d %s" % (j, x), v[i], bars[x][0]) for j, v in joints.items() for i, x in enumerate(("q", "qd"))]
    return S.compare(case, ref, out, label, report=report, p99=p99, elements=elements)


def report_line(name, ref, err, outliers, bars, joints):
    """one line of the report: step_terms.report_words with the worst aimed-joint errors before the raised bars, then the kept envs
    per regime (and how many show it)"""
    words = S.report_words(name, 34, ref, err, outliers, bars)
    if joints:
        words.insert(-1, "aimed_q=%.1e aimed_qd=%.1e" % (max(v[0] for v in joints.values()), max(v[1] for v in joints.values())))
    words.append("regimes: " + " ".join("%s=%d(%d)" % (nm, a, b) for nm, (a, b) in regime_counts(ref).items()))
    return "  ".join(words)


# ---------------------------------------------------------------------------------------------------------------- planted slips
SLIPS = ("limit_k", "limit_d", "joint_friction", "jfric_veps", "armature", "effort", "vel_limit", "kp_scale_ignored", "kd_scale_ignored",
         "lo_from_model", "hi_from_model", "lock_sign")
_SCALED = {"limit_k": 0.8, "limit_d": 0.5, "joint_friction": 0.8, "jfric_veps": 2.0, "armature": 0.8, "effort": 0.95, "vel_limit": 0.98}
_DROPPED = {"kp_scale_ignored": abi.PARAM_KP_SCALE, "kd_scale_ignored": abi.PARAM_KD_SCALE, "lo_from_model": abi.PARAM_DOF_LOWER,
            "hi_from_model": abi.PARAM_DOF_UPPER}
# the cases each slip is looked for in, the likeliest first: (scenario, asset, n, substeps, dr)
SLIP_CASES = {"limit_k": ("limits",), "limit_d": ("limits",), "joint_friction": ("friction",), "jfric_veps": ("friction",),
              "armature": ("drive",), "effort": ("drive",), "vel_limit": ("drive",), "lock_sign": ("drive",)}


def planted(slip):
    """(ref, outputs): a case and the fp32 build's outputs of the same case with one thing made wrong -- on the oracle side only, no
    kernel is edited.
      limit_k x 0.8, limit_d x 0.5                                        limits, plain: in the config
      joint_friction x 0.8, jfric_veps x 2                                friction: in the config
      armature x 0.8, effort x 0.95, vel_limit x 0.98                     drive: in the config
      kp_scale_ignored, kd_scale_ignored, lo_from_model, hi_from_model    limits, dr: the per-env parameter is not handed to the oracle
      lock_sign                                                           drive: every lock the predictor takes is forced onto the opposite
                                                                          limit through dynamics_x's force_lock (tune[22] = -1, oracle only)"""
    assert slip in SLIPS
    if slip in _DROPPED:
        base = ("limits", "default", N, 2, True)

        def wrong(cfg, params, p=_DROPPED[slip]):
            del params[p]
            return params
    else:
        base = (SLIP_CASES[slip][0], "default", N, 2, False)

        def wrong(cfg, params):
            if slip == "lock_sign":
                cfg.tune[22] = -1.0
            else:
                setattr(cfg, slip, getattr(cfg, slip) * _SCALED[slip])
            return params
    return reference(*base), reference(*base, wrong=wrong, tag=slip).out32
