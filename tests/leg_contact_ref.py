"""Leg <-> leg capsule contact of the fused step, pair by pair: state generators that put every one of the 28 left-leg x right-leg
capsule pairs into contact within the model's joint limits, the numpy side (the fp64 pair geometry of tests/proximity_numpy.py), and
the oracle's side, the comparison and the planted slips of tests/test_leg_contact_cpu.py and tests/test_gpu_leg_contact.py (on the harness
of tests/step_terms.py).

The pair geometry does not depend on the root's attitude nor on the arm and head joints, so the postures are searched once per process
(`pool`) with the root at the identity and shared by every scenario and asset (the leg geometry of the three assets is the same table:
tests/test_leg_contact_cpu.py).  Scenarios (`case_states`):
  free        zero gravity, root at z = 1 with a random attitude, env e aims at pair e % 28: the aimed pair overlaps by 1 - 10 mm, at most
              three pairs overlap, none by more than 15 mm, no pair within 0.2 mm of touching, no overlapping pair nearly parallel
  solo        the free states whose aimed pair is the only overlapping one; the other envs stand with default leg joints (no overlap)
  both_parts  a pair owned by part 0 of the wave kernels (left hip, thigh, calf capsule) and one owned by part 1 (left ankle and the two
              foot-plate capsules) overlap at once, up to five pairs; first the envs in which both foot-plate capsules of one foot touch
              the other leg (one link receives two wrenches)
  stance      the reset state on the ground under gravity with both hip rolls turned inward
  sparse      free with default leg joints everywhere except step_terms.NEIGHBOUR_ENVS"""
import numpy as np

from bez_isaacgym_amd import abi
from tests import ball_contact_ref as B
from tests import proximity_numpy as P
from tests import step_terms as S

NPAIR = P.NPAIR
LEGS = list(range(4, 10)) + list(range(12, 18))
HIP_ROLLS = (5, 13)
KEPT_MARGIN = 1e-4        # m: a pair this close to touching may be decided either way by two roundings (DESIGN.md 6 "knife edges")
CLEAR = 2e-4              # m: the generators leave no pair closer to touching than this
AIM_DEPTH = (1e-3, 10e-3)
MAX_DEPTH = 15e-3
LIMIT_MARGIN = 0.03       # rad: the postures stay this far inside the joint limits (a step moves a joint by up to 1 rad/s x dt)
PER_PAIR = 36             # postures searched per pair: 1000 envs aim 35 - 36 at each
SOLO_FIRST = 18           # of which up to this many solo ones are taken first
DRAWS = 100000
PARKED_BALL = (0.0, 3.0, 1.0)
STANCE_BALL = (0.0, 3.0)
SLOW_LEGS = 0.05          # in three envs of four the leg joints' speeds are scaled by this: a separating speed rejects a contact

_T = P.tables("default")
_IA, _IB = _T["pairs"][:, 0], _T["pairs"][:, 1]
PART = (_IA > 2).astype(int)            # owner of a pair in the wave kernels: 0 = left hip / thigh / calf capsule, 1 = left ankle / foot plates
LEFT_PLATES, RIGHT_PLATES = (4, 5), (10, 11)


def pair_bodies(asset):
    """(28, 2) body rows of the two capsules of every pair, from the model JSON (capsule -> link -> body of the asset)"""
    links = B.asset_links(asset)
    body = np.array([int(links[l]["body"]) for l in _T["cap_link"]])
    return np.stack([body[_IA], body[_IB]], 1)


def pair_geometry(root_quat, q, asset="default"):
    """fp64 (gap (n, 28), sin^2 of the angle between the axes (n, 28), normal b -> a (n, 28, 3)) of the fp32 state"""
    T = P.tables(asset)
    E, r = P.link_frames(T, np.asarray(root_quat, np.float32), np.asarray(q, np.float32), np.float64)
    c0, c1 = P.capsule_axes(T, E, r, np.float64)
    d1, d2 = c1[:, _IA] - c0[:, _IA], c1[:, _IB] - c0[:, _IB]
    rows = P.pair_rows(T, c0, c1, np.zeros((len(q), 3)), np.float64)
    cr = np.cross(d1, d2)
    sin2 = (cr * cr).sum(-1) / ((d1 * d1).sum(-1) * (d2 * d2).sum(-1))
    return rows[:, :, P.GAP], sin2, rows[:, :, P.NORMAL]


def _identity(n):
    quat = np.zeros((n, 4)); quat[:, 3] = 1.0
    return quat


def accepted(gap, sin2, max_pairs):
    """draws that meet the conditions every scenario shares"""
    ov = gap < 0
    return ((ov.sum(1) <= max_pairs) & (gap.min(1) >= -MAX_DEPTH) & (np.abs(gap) >= CLEAR).all(1)
            & ~(ov & (sin2 < P.PAIR_MIN_SIN2)).any(1))


def aimed_ok(gap, p):
    return (gap[:, p] <= -AIM_DEPTH[0]) & (gap[:, p] >= -AIM_DEPTH[1])


def plates_both(gap):
    """draws in which both foot-plate capsules of one foot overlap capsules of the other leg"""
    ov = gap < 0
    left = ov[:, _IA == LEFT_PLATES[0]].any(1) & ov[:, _IA == LEFT_PLATES[1]].any(1)
    right = ov[:, _IB == RIGHT_PLATES[0]].any(1) & ov[:, _IB == RIGHT_PLATES[1]].any(1)
    return left | right


def parts_both(gap):
    ov = gap < 0
    return ov[:, PART == 0].any(1) & ov[:, PART == 1].any(1)


def _limits():
    lo, hi = np.asarray(P.MODEL["dof_lower"], np.float64), np.asarray(P.MODEL["dof_upper"], np.float64)
    return lo[LEGS] + LIMIT_MARGIN, hi[LEGS] - LIMIT_MARGIN


def _geom_legs(legs):
    q = np.tile(np.asarray(P.MODEL["dof_default"], np.float64), (len(legs), 1))
    q[:, LEGS] = legs
    gap, sin2, _ = pair_geometry(_identity(len(q)), q)
    return gap, sin2


_POOL = None


def pool(seed=0):
    """The leg postures of every scenario, searched once per process: DRAWS uniform draws of the twelve leg joints inside their limits,
    and for the pairs they reach fewer than PER_PAIR times (or fewer than 5 times alone) a local search around the postures found
    (Gaussian steps of 0.04 rad, clipped to the limits, accepted by the same conditions).
    -> dict(legs {pair: (k, 12) fp32}, solo {pair: (k,) bool}, both_legs (m, 12) fp32 with the plates_both draws first, both_plates (m,) bool)"""
    global _POOL
    if _POOL is not None:
        return _POOL
    rng = np.random.default_rng(seed)
    lo, hi = _limits()
    draws = rng.uniform(lo, hi, (DRAWS, 12)).astype(np.float32)
    gap, sin2 = _geom_legs(draws)
    ok3 = accepted(gap, sin2, 3)
    alone = (gap < 0).sum(1) == 1
    legs, solo = {}, {}
    for p in range(NPAIR):
        cand = ok3 & aimed_ok(gap, p)
        have, have_solo = draws[cand], alone[cand]
        if len(have) == 0:   # no draw met the conditions: start from the draws whose pair p is nearest the middle of the aimed depth
            order = np.argsort(np.abs(gap[:, p] + 0.5 * (AIM_DEPTH[0] + AIM_DEPTH[1])))[:20]
            seeds = draws[order]
        else:
            seeds = have
        for _ in range(12):
            if len(have) >= PER_PAIR and have_solo.sum() >= 5:
                break
            base = seeds[rng.integers(0, len(seeds), 1500)]
            trial = np.clip(base + rng.normal(0.0, 0.04, base.shape), lo, hi).astype(np.float32)
            g, s2 = _geom_legs(trial)
            good = accepted(g, s2, 3) & aimed_ok(g, p)
            if len(have) >= PER_PAIR:
                good &= (g < 0).sum(1) == 1
            have = np.concatenate([have, trial[good]]); have_solo = np.concatenate([have_solo, ((g < 0).sum(1) == 1)[good]])
            if len(have):
                seeds = have
        # up to SOLO_FIRST solo postures first, then the others, then the remaining solo ones
        s, o = np.flatnonzero(have_solo), np.flatnonzero(~have_solo)
        order = np.concatenate([s[:SOLO_FIRST], o, s[SOLO_FIRST:]])[:PER_PAIR]
        legs[p], solo[p] = have[order], have_solo[order]
    ok5 = accepted(gap, sin2, 5) & parts_both(gap) & ((gap <= -AIM_DEPTH[0]) & (gap >= -AIM_DEPTH[1])).any(1)
    pl = ok5 & plates_both(gap)
    idx = np.concatenate([np.flatnonzero(pl)[:200], np.flatnonzero(ok5 & ~pl)])
    _POOL = dict(legs=legs, solo=solo, both_legs=draws[idx], both_plates=pl[idx])
    return _POOL


# ---------------------------------------------------------------------------------------------------------------- generators
def _free_body(n, seed):
    """zero-gravity states without the legs: root at z = 1 with a random attitude and the velocities of ball_contact_ref.free_space_states,
    arm and head joints at default +- 0.3 rad, joint speeds U(-1, 1) with the leg joints' scaled by SLOW_LEGS in three envs of four, the
    ball at rest at PARKED_BALL"""
    rng = np.random.default_rng(seed)
    dflt = np.asarray(P.MODEL["dof_default"], np.float64)
    rs = np.zeros((n, 2, 13)); ds = np.zeros((n, 18, 2))
    quat = rng.normal(size=(n, 4)); quat /= np.linalg.norm(quat, axis=1, keepdims=True)
    rs[:, 0, 2] = 1.0
    rs[:, 0, 3:7] = quat
    rs[:, 0, 7:10] = rng.uniform(-0.3, 0.3, (n, 3))
    rs[:, 0, 10:13] = rng.uniform(-1.0, 1.0, (n, 3))
    ds[:, :, 0] = dflt + rng.uniform(-0.3, 0.3, (n, 18))
    ds[:, LEGS, 0] = dflt[LEGS]
    ds[:, :, 1] = rng.uniform(-1.0, 1.0, (n, 18))
    slow = (np.arange(n) // NPAIR) % 4 != 3
    ds[np.ix_(slow, LEGS, [1])] *= SLOW_LEGS
    rs[:, 1, 0:3] = PARKED_BALL
    rs[:, 1, 6] = 1.0
    return rs, ds


def free_states(n, seed=4):
    """env e aims at pair e % 28 with the (e // 28)-th posture of the pair's pool"""
    rs, ds = _free_body(n, seed)
    pl = pool()
    aim = np.arange(n) % NPAIR
    solo = np.zeros(n, bool)
    for e in range(n):
        k = (e // NPAIR) % len(pl["legs"][aim[e]])
        ds[e, LEGS, 0] = pl["legs"][aim[e]][k]
        solo[e] = pl["solo"][aim[e]][k]
    return dict(root_states=rs.astype(np.float32), dof_state=ds.astype(np.float32), aim=aim, solo=solo)


def default_legs(states, keep):
    """a copy of `states` with default leg joints (no pair overlaps) in every env that is not marked in `keep`; aim -1 there"""
    ds = states["dof_state"].copy()
    away = ~np.asarray(keep, bool)
    ds[np.ix_(away, LEGS, [0])] = np.asarray(P.MODEL["dof_default"], np.float32)[LEGS][None, :, None]
    return dict(states, dof_state=ds, aim=np.where(away, -1, states["aim"]))


def both_parts_states(n, seed=5):
    rs, ds = _free_body(n, seed)
    pl = pool()
    k = np.arange(n) % len(pl["both_legs"])
    ds[:, LEGS, 0] = pl["both_legs"][k]
    st = dict(root_states=rs.astype(np.float32), dof_state=ds.astype(np.float32), plates=pl["both_plates"][k])
    gap, _, _ = pair_geometry(st["root_states"][:, 0, 3:7], st["dof_state"][:, :, 0])
    st["aim"] = gap.argmin(1)   # the deepest pair
    return st


def stance_states(n, asset, seed=6):
    """the reset state of step_terms.step_cfg(n, asset) (standing on the ground under gravity) with both hip rolls turned inward by U(0, 0.17) rad,
    joint speeds U(-0.3, 0.3), the ball at rest 1 mm into the ground at STANCE_BALL"""
    from oracle.bez_oracle import Oracle
    rng = np.random.default_rng(seed)
    fresh = Oracle(S.step_cfg(n, asset))
    rs = np.asarray(fresh.root_states, np.float64).reshape(n, 2, 13).copy()
    ds = np.asarray(fresh.dof_state, np.float64).reshape(n, 18, 2).copy()
    ds[:, HIP_ROLLS[0], 0] += HIP_ROLL_INWARD[0] * rng.uniform(0.0, 0.17, n)
    ds[:, HIP_ROLLS[1], 0] += HIP_ROLL_INWARD[1] * rng.uniform(0.0, 0.17, n)
    ds[:, :, 1] = rng.uniform(-0.3, 0.3, (n, 18))
    rs[:, 1, :] = 0.0
    rs[:, 1, 0:2] = STANCE_BALL
    rs[:, 1, 2] = B.ball_radius() - 1e-3
    rs[:, 1, 6] = 1.0
    st = dict(root_states=rs.astype(np.float32), dof_state=ds.astype(np.float32))
    gap, _, _ = pair_geometry(st["root_states"][:, 0, 3:7], st["dof_state"][:, :, 0])
    st["aim"] = np.where(gap.min(1) < 0, gap.argmin(1), -1)
    return st


HIP_ROLL_INWARD = (-1.0, -1.0)  # sign of the left / right hip roll that brings the legs together (tests/test_leg_contact_cpu.py)


def case_states(scenario, asset, n):
    if scenario == "stance":
        return stance_states(n, asset)
    if scenario == "both_parts":
        return both_parts_states(n)
    st = free_states(n)
    if scenario == "solo":
        return default_legs(st, st["solo"])
    if scenario == "sparse":
        keep = np.zeros(n, bool); keep[list(S.NEIGHBOUR_ENVS)] = True
        return default_legs(st, keep)
    assert scenario == "free", scenario
    return st


def kept(gap):
    """envs in which no pair is within KEPT_MARGIN of touching"""
    return (np.abs(gap) >= KEPT_MARGIN).all(1)


# ---------------------------------------------------------------------------------------------------------------- momentum
def momentum_change(before, after):
    """(n, 2): largest component of the change of the robot's linear momentum (kg m/s) and of its angular momentum about its centre
    of mass (kg m^2/s), between two step_terms.robot_momentum"""
    return np.stack([np.abs(after[0] - before[0]).max(1), np.abs(after[1] - before[1]).max(1)], 1)


# ---------------------------------------------------------------------------------------------------------------- the oracle's side of a case
def reference(scenario, asset, n, substeps=2, dr=False, flags=0):
    """step_terms.reference of a leg case: states, per-env parameters, actions, the numpy pair geometry of the start state, kept, both
    outputs, the momentum change."""
    def build(ref):
        ref.cfg = lambda: S.step_cfg(n, asset, gravity=(scenario == "stance"), substeps=substeps, flags=flags)
        ref.states = case_states(scenario, asset, n)
        ref.aim = ref.states["aim"]
        ref.params = S.dr_params(n, 8) if dr else None
        ref.actions = S.actions(n, 2)
        ref.gap, ref.sin2, ref.normal = pair_geometry(ref.states["root_states"][:, 0, 3:7], ref.states["dof_state"][:, :, 0], asset)
        ref.kept = kept(ref.gap)
        pair = S.oracle_pair(ref)
        before = [S.robot_momentum(o, n, asset) for o in pair]
        S.step_pair(ref, *pair)
        ref.dp64, ref.dp32 = (momentum_change(b, S.robot_momentum(o, n, asset)) for b, o in zip(before, pair))
    return S.reference(("leg", scenario, asset, n, substeps, dr, flags), build,
                       scenario=scenario, asset=asset, n=n, substeps=substeps, dr=dr, flags=flags)


NS = abi.FLAG_NO_SELF_COLLISION
NS_SHARE = 0.5
N = S.N
# every oracle case of tests/test_gpu_leg_contact.py: (scenario, asset, n, substeps, dr, flags)
CASES = ([("free", a, N, 2, dr, 0) for a in S.ASSETS for dr in (False, True)]
         + [("solo", a, N, 1, False, f) for a in ("default", "cleats") for f in (0, abi.FLAG_CF_WITH_FRICTION)]
         + [("both_parts", "default", N, s, False, 0) for s in (1, 2, 3, 4)]
         + [("stance", a, N, 2, False, 0) for a in S.ASSETS]
         + [("free", "default", 200, 2, False, 0), ("sparse", "default", 200, 2, False, 0), ("free", "default", N, 2, False, NS)])


def case_name(scenario, asset, n, substeps, dr, flags):
    return "%s%s-s%d%s%s %s" % (scenario, "" if n == N else str(n), substeps, "-dr" if dr else "",
                                "-ns" if flags & NS else "-fric" if flags & abi.FLAG_CF_WITH_FRICTION else "", asset)


def aimed_rows(cf, ref):
    """(n, 2, 3) the contact-force rows of the aimed pair's two bodies (zeros where the env aims at nothing)"""
    n = ref.n
    rows = np.asarray(cf).reshape(n, -1, 3)
    pb = pair_bodies(ref.asset)[np.maximum(ref.aim, 0)]
    out = rows[np.arange(n)[:, None], pb]
    out[ref.aim < 0] = 0.0
    return out


def compare(case, ref, out, label, report=None, p99=True):
    """step_terms.compare, and per aimed pair the worst contact-force error of its kept envs outside the outliers within the cf bar"""
    return S.compare(case, ref, out, label, report=report, p99=p99,
                     elements=lambda bars, bad: ((), S.aimed_cf_checks(ref, out, bars, bad, NPAIR, "pair")))


def normal_tolerance(ref):
    """3 x the worst error of the pair normals of proximity_numpy.pair_rows evaluated in np.float32 against fp64 on the states of `ref`,
    over the aimed pairs that proximity_numpy.conditioning calls pair_ok"""
    rs, ds = ref.states["root_states"], ref.states["dof_state"]
    T = P.tables(ref.asset)
    E, r = P.link_frames(T, rs[:, 0, 3:7], ds[:, :, 0], np.float32)
    c0, c1 = P.capsule_axes(T, E, r, np.float32)
    n32 = P.pair_rows(T, c0, c1, np.zeros((ref.n, 3), np.float32), np.float32)[:, :, P.NORMAL].astype(np.float64)
    ok = P.conditioning(ref.asset, rs[:, 0], ds, rs[:, 1, 0:3])["pair_ok"]
    e = np.flatnonzero(ref.aim >= 0)
    sel = ok[e, ref.aim[e]]
    err = np.abs(n32[e, ref.aim[e]] - ref.normal[e, ref.aim[e]]).max(1)
    return 3.0 * float(err[sel].max()), ok


# ---------------------------------------------------------------------------------------------------------------- planted slips
SLIPS = ("pair_dropped", "scale_from_part0", "row_sign")
SLIP_PAIR = 16   # left ankle capsule x right first foot-plate capsule


def planted(slip):
    """(ref, outputs): a case and a copy of its fp32 build's outputs with one slip planted -- on the oracle side only, no kernel is edited.
      pair_dropped      solo, 2 substeps: the envs aimed at SLIP_PAIR step as the oracle steps them with BEZ_FLAG_NO_SELF_COLLISION; the
                        aimed pair is the only one that overlaps there, so this is exactly that pair's force left out (by config)
      scale_from_part0  both_parts, 1 substep: the oracle's config cannot take the scale s from one part's sum of |f|^2, so it is planted
                        in the outputs.  At one substep pose, root velocity, q and qd are linear in s: x = x_off + s d.  They are moved to
                        x_off + phi (x - x_off), x_off from the oracle with the contact switched off, phi = part 0's share of the sum of
                        depth^2 over the overlapping pairs (the share of the spring forces' squares, which stands for that of |f|^2)
      row_sign          solo, 2 substeps: the contact-force row of capsule b's body negated in the envs aimed at SLIP_PAIR (in the outputs)"""
    assert slip in SLIPS
    if slip == "scale_from_part0":
        ref, off = reference("both_parts", "default", N, substeps=1), reference("both_parts", "default", N, substeps=1, flags=NS)
        out = {k: v.copy() for k, v in ref.out32.items()}
        d2 = np.where(ref.gap < 0, ref.gap, 0.0) ** 2
        phi = (d2[:, PART == 0].sum(1) / d2.sum(1))[:, None]
        for k in ("pose", "root_vel", "q", "qd"):
            out[k] = off.out32[k] + phi * (ref.out32[k] - off.out32[k])
        return ref, out
    ref = reference("solo", "default", N, substeps=2)
    out = {k: v.copy() for k, v in ref.out32.items()}
    envs = ref.aim == SLIP_PAIR
    if slip == "pair_dropped":
        off = reference("solo", "default", N, substeps=2, flags=NS)
        for k in out:
            out[k][envs] = off.out32[k][envs]
    else:
        cf = out["cf"].reshape(ref.n, -1, 3)
        cf[envs, pair_bodies(ref.asset)[SLIP_PAIR, 1]] *= -1.0
    return ref, out
