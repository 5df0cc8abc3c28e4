"""Ground contact of the fused step, point by point: state generators that put every one of the 22 ground points (8 foot corners or
cleats, 8 torso, 4 head and 2 forearm guard points; bez_model.json "ground_points") under the plane, the numpy side (depth, normal
force at the start of the step, active set, tangential speed and friction regime of every point, from the model JSON and the
Isaac-visible rows alone), and the oracle's side, the comparison and the planted slips of tests/test_ground_contact_cpu.py and
tests/test_gpu_ground_contact.py (on the harness of tests/step_terms.py).

The contact law: a point at depth d > 0 whose fn0 = kn d - (h kn + cn) v_z is positive is a spring-damper, integrated
implicitly, with the tangential viscosity ct = min(mu fn0 / max(vt, veps), ct_max).  Three friction regimes: slipping (vt > veps, under
the cap), capped (ct = ct_max) and inside veps under the cap.  Scenarios (`case_states`):
  free        zero gravity, random torso attitude, all 18 joints anywhere inside their limits; env e has ground point e % 22 alone under
              the plane by 0.5 - 10 mm, every other point at least CLEAR above it, no leg pair closer than CLEAR; every fourth block of 22
              envs moves at 0.02 x the speed (the slow friction regimes); the ball lies 3 m away, 0.5 - 5 mm into the ground, rolling
  solo        the free states (run at one substep, for the row checks)
  lying       default gravity, the robot on its front, back, left or right side within 0.25 rad, joints default +- 1 rad: at least two
              points of at least two bodies under the plane, the lowest by 1 - 8 mm
  torso_ball  lying on the front or back with a torso point under the plane and the ball 0.5 - 10 mm into the torso box from above
  sparse      free with the robot and the ball lifted 0.5 m clear of the ground everywhere except step_terms.NEIGHBOUR_ENVS"""
import numpy as np

from bez_isaacgym_amd import abi
from tests import proximity_numpy as P
from tests import ball_contact_ref as B
from tests import step_terms as S
from tests.leg_contact_ref import pair_geometry, CLEAR
from tests.proximity_numpy import tables, link_frames

NPT = P.NPT
BALL = NPT                # the ball's column in the per-point terms
KEPT_MARGIN = 1e-4        # m: a point this close to the plane, or to fn0 = 0, may be decided either way by two roundings (DESIGN.md 6 "knife edges")
LIMIT_MARGIN = 0.03       # rad: the postures stay this far inside the joint limits
AIM_DEPTH = (0.5e-3, 10e-3)
BALL_DEPTH = (0.5e-3, 5e-3)
LYING_DEPTH = (1e-3, 8e-3)
BALL_AWAY = 3.0           # m
LIFT = 0.5                # m
SLOW = 0.02               # every fourth block of 22 envs moves at this share of the speeds
LYING_SPEED = 0.25        # the lying scenarios move at this share of free's speeds
PER_POINT = 46            # postures per point: 1000 envs aim 45 - 46 at each
CHUNK = 20000
N = S.N
NONE, SLIPPING, CAPPED, INSIDE = 0, 1, 2, 3
REGIMES = {SLIPPING: "slipping", CAPPED: "capped", INSIDE: "inside_veps"}
GRAVITY = ("lying", "torso_ball")
# the non-default contact parameters of the "params" case: with ct_max veps / mu = 80 N and kn d = 7.5 - 150 N the slow envs split
# between the capped regime and the one inside veps under the cap, which the default parameters (10 N) never reach at >= 0.5 mm
PARAMS = (("contact_kn", 1.5e4), ("contact_cn", 30.0), ("contact_ct", 4.0e3), ("contact_veps", 0.02), ("ball_kn", 1.2e4), ("ball_cn", 60.0))
BODIES = ("torso", "head", "forearm", "foot")


def point_bodies(asset):
    """(22,) body row of every ground point (the cleats asset: the cleat's own row, not the foot plate's)"""
    m = P.MODEL
    pts = (m["cleats"] if asset == "cleats" else m)["ground_points"]
    return np.array([int(p["body"]) for p in pts])


def point_group(asset="default"):
    """(22,) index into BODIES of every point: which of torso / head / forearm / foot carries it"""
    names = [P.MODEL["links"][l]["name"] for l in tables(asset)["pt_link"]]
    return np.array([[k for k, b in enumerate(BODIES) if b in nm][0] for nm in names])


def foot_plate_rows(asset):
    return [B.box_table(asset)[b]["body"] for b in (4, 9)]


def points_rel(asset, root_quat, q):
    """fp64 (n, 22, 3) positions of the ground points relative to the root origin, from the fp32 state"""
    T = tables(asset)
    E, r = link_frames(T, np.asarray(root_quat, np.float32), np.asarray(q, np.float32), np.float64)
    l = T["pt_link"]
    return r[:, l] + np.einsum("nlij,lj->nli", E[:, l], T["pt_pos"])


def heights(states, asset):
    """fp64 (n, 23): height of the 22 ground points and of the ball's lowest point above the plane"""
    rs = states["root_states"].astype(np.float64)
    z = rs[:, 0, 2:3] + points_rel(asset, states["root_states"][:, 0, 3:7], states["dof_state"][:, :, 0])[:, :, 2]
    return np.concatenate([z, rs[:, 1, 2:3] - B.ball_radius()], 1)


def contact_values(cfg):
    """the contact law's constants as the step resolves them"""
    kn, cn = float(cfg.contact_kn), float(cfg.contact_cn)
    return dict(kn=kn, cn=cn, ct=float(cfg.contact_ct), veps=float(cfg.contact_veps), bkn=float(cfg.ball_kn) if cfg.ball_kn > 0 else kn,
                bcn=float(cfg.ball_cn) if cfg.ball_cn > 0 else cn, h=float(cfg.dt) / int(cfg.substeps), mu=float(cfg.plane_friction))


def terms(states, asset, rb, cfg, friction=None):
    """The start state's contact terms per point (column 22: the ball), fp64, from the model JSON, the state tensors and the rigid-body
    rows rb (n, rows, 13) -- a point's velocity is its body row's v + w x (x - x_row):
    height, d, vel (n, 23, 3), fn0, active (d > 0 and fn0 > 0), vt, regime (NONE where inactive)"""
    c = contact_values(cfg)
    rs = states["root_states"].astype(np.float64)
    rb = np.asarray(rb, np.float64)
    n = len(rs)
    x = rs[:, 0:1, 0:3] + points_rel(asset, states["root_states"][:, 0, 3:7], states["dof_state"][:, :, 0])
    rows = rb[:, point_bodies(asset)]
    vel = rows[:, :, 7:10] + np.cross(rows[:, :, 10:13], x - rows[:, :, 0:3])
    R = B.ball_radius()
    ball = rb[:, B.ball_row(asset)]
    vball = ball[:, 7:10] + np.cross(ball[:, 10:13], np.array([0.0, 0.0, -R]))
    vel = np.concatenate([vel, vball[:, None]], 1)
    height = np.concatenate([x[:, :, 2], ball[:, 2:3] - R], 1)
    kn = np.r_[np.full(NPT, c["kn"]), c["bkn"]]
    cn = np.r_[np.full(NPT, c["cn"]), c["bcn"]]
    mu = np.full((n, 1), c["mu"]) if friction is None else np.asarray(friction, np.float64).reshape(n, 1)
    d = -height
    fn0 = kn * d - (c["h"] * kn + cn) * vel[:, :, 2]
    active = (d > 0) & (fn0 > 0)
    vt = np.hypot(vel[:, :, 0], vel[:, :, 1])
    raw = mu * fn0 / np.maximum(vt, c["veps"])
    regime = np.where(raw >= c["ct"], CAPPED, np.where(vt > c["veps"], SLIPPING, INSIDE))
    return dict(height=height, d=d, vel=vel, fn0=fn0, kn=kn, active=active, vt=vt, regime=np.where(active, regime, NONE))


def kept(t):
    """envs in which no point is within KEPT_MARGIN of the plane and no point under the plane within KEPT_MARGIN x kn of fn0 = 0"""
    edge = (np.abs(t["d"]) <= KEPT_MARGIN) | ((t["d"] > 0) & (np.abs(t["fn0"]) / t["kn"] <= KEPT_MARGIN))
    return ~edge.any(1)


def regime_counts(t, rows):
    """{regime name: number of the envs `rows` in which some robot point is in it}"""
    return {name: int((t["regime"][rows][:, :NPT] == r).any(1).sum()) for r, name in REGIMES.items()}


def active_bodies(t, asset):
    """(n, robot bodies + 1) bool: the rows the active set loads (the last column: the ball's)"""
    nb = B.ball_row(asset)
    out = np.zeros((len(t["active"]), nb + 1), bool)
    pb = np.r_[point_bodies(asset), nb]
    for i in range(NPT + 1):
        out[:, pb[i]] |= t["active"][:, i]
    return out


# ---------------------------------------------------------------------------------------------------------------- posture pools
def _limits():
    return (np.asarray(P.MODEL["dof_lower"], np.float64) + LIMIT_MARGIN, np.asarray(P.MODEL["dof_upper"], np.float64) - LIMIT_MARGIN)


def _legs_clear(asset, quat, q):
    gap, _, _ = pair_geometry(quat, q, asset)
    return gap.min(1) >= CLEAR


def _quat_mul(a, b):
    """xyzw: the rotation b followed by a"""
    ax, ay, az, aw = (a[..., k] for k in range(4)); bx, by, bz, bw = (b[..., k] for k in range(4))
    return np.stack([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz], -1)


_POOLS = {}


def free_pool(asset, seed=0):
    """Per ground point PER_POINT postures (root quaternion, joints, root height; fp32) in which the point is under the plane alone:
    uniform attitudes and joints in chunks of CHUNK draws, each with its own depth, kept where the second-lowest point clears the plane
    by CLEAR and the leg pairs clear each other.  -> {point: (quat (k, 4), q (k, 18), z (k,))}"""
    key = ("free", asset)
    if key in _POOLS:
        return _POOLS[key]
    rng = np.random.default_rng(seed)
    lo, hi = _limits()
    have = {p: [] for p in range(NPT)}
    count = np.zeros(NPT, int)
    for _ in range(40):
        if count.min() >= PER_POINT:
            break
        quat = rng.normal(size=(CHUNK, 4)); quat = (quat / np.linalg.norm(quat, axis=1, keepdims=True)).astype(np.float32)
        q = rng.uniform(lo, hi, (CHUNK, 18)).astype(np.float32)
        depth = rng.uniform(*AIM_DEPTH, CHUNK)
        z = points_rel(asset, quat, q)[:, :, 2]
        two = np.partition(z, 1, axis=1)
        low = z.argmin(1)
        ok = np.flatnonzero((two[:, 1] - two[:, 0] >= depth + CLEAR) & (count[low] < PER_POINT))
        ok = ok[_legs_clear(asset, quat[ok], q[ok])]
        for i in ok:
            if count[low[i]] < PER_POINT:
                have[low[i]].append((quat[i], q[i], np.float32(-depth[i] - two[i, 0]))); count[low[i]] += 1
    assert count.min() >= PER_POINT, count
    _POOLS[key] = {p: tuple(np.stack([h[k] for h in have[p]]) for k in range(3)) for p in range(NPT)}
    return _POOLS[key]


_SIDES = np.array([[0.0, np.sin(np.pi / 4), 0.0, np.cos(np.pi / 4)],     # front: the torso's x axis points down
                   [0.0, -np.sin(np.pi / 4), 0.0, np.cos(np.pi / 4)],    # back
                   [-np.sin(np.pi / 4), 0.0, 0.0, np.cos(np.pi / 4)],    # left side: the y axis points down
                   [np.sin(np.pi / 4), 0.0, 0.0, np.cos(np.pi / 4)]])    # right side
LYING_COMBOS = ((0, 1), (0, 2), (1, 2))   # torso + head, torso + forearm, head + forearm (indices into BODIES)
LYING_QUOTA = 130
LYING_PER_POINT = 30


def lying_pool(asset, n=N, seed=1):
    """2.5 n accepted lying draws: at least two points of at least two bodies under the plane, no point within CLEAR of it, the leg
    pairs clear.  -> dict(quat, q, z (fp32), side (0 front, 1 back, 2 left, 3 right), under (m, 22) bool)"""
    key = ("lying", asset, n)
    if key in _POOLS:
        return _POOLS[key]
    rng = np.random.default_rng(seed)
    lo, hi = _limits()
    dflt = np.asarray(P.MODEL["dof_default"], np.float64)
    link = tables(asset)["pt_link"]
    got = dict(quat=[], q=[], z=[], side=[], under=[])
    total = 0
    for _ in range(40):
        if total >= int(2.5 * n):
            break
        side = rng.integers(0, 4, CHUNK)
        axis = rng.normal(size=(CHUNK, 3)); axis /= np.linalg.norm(axis, axis=1, keepdims=True)
        ang = rng.uniform(0.0, 0.25, CHUNK)
        extra = np.concatenate([axis * np.sin(0.5 * ang)[:, None], np.cos(0.5 * ang)[:, None]], 1)
        quat = _quat_mul(extra, _SIDES[side]).astype(np.float32)
        q = np.clip(dflt + rng.uniform(-1.0, 1.0, (CHUNK, 18)), lo, hi).astype(np.float32)
        depth = rng.uniform(*LYING_DEPTH, CHUNK)
        rel = points_rel(asset, quat, q)[:, :, 2]
        z = (-depth - rel.min(1)).astype(np.float32)
        h = z[:, None].astype(np.float64) + rel
        under = h < 0
        nbody = sum(under[:, link == l].any(1).astype(int) for l in np.unique(link))
        ok =np.flatnonzero((under.sum(1) >= 2) & (nbody >= 2) & (np.abs(h) >= CLEAR).all(1))
        ok = ok[_legs_clear(asset, quat[ok], q[ok])]
        for k, v in (("quat", quat), ("q", q), ("z", z), ("side", side), ("under", under)):
            got[k].append(v[ok])
        total += len(ok)
    assert total >= int(2.5 * n), total
    _POOLS[key] = {k: np.concatenate(v) for k, v in got.items()}
    return _POOLS[key]


def under_bodies(under, asset="default"):
    """(m, 4) bool: which of torso / head / forearm / foot has a point under the plane"""
    grp = point_group(asset)
    return np.stack([(under & (grp == b)).any(1) for b in range(len(BODIES))], 1)


def lying_selection(pool, n, asset):
    """indices of n pool draws: first LYING_QUOTA of each of the three upper-body pairs (exactly those two of torso / head / forearm
    and no foot), then draws for the points still under the plane in fewer than LYING_PER_POINT envs, then the others in the order drawn"""
    ub = under_bodies(pool["under"], asset)
    first = []
    for a, b in LYING_COMBOS:
        exact = ub[:, a] & ub[:, b] & (ub.sum(1) == 2)
        first.extend(np.flatnonzero(exact)[:LYING_QUOTA * n // N].tolist())
    taken = np.zeros(len(ub), bool); taken[first] = True
    for p in np.argsort(pool["under"].sum(0)):   # then, rarest point first, draws until every point is under the plane in LYING_PER_POINT
        more = np.flatnonzero(pool["under"][:, p] & ~taken)[:max(0, LYING_PER_POINT * n // N - int(pool["under"][taken, p].sum()))]
        first.extend(more.tolist()); taken[more] = True
    rest = np.flatnonzero(~taken)
    return np.array((first + rest.tolist())[:n])


# ---------------------------------------------------------------------------------------------------------------- generators
def _ball_on_ground(rs, rng, scale):
    n = len(rs)
    rs[:, 1, :] = 0.0
    rs[:, 1, 0] = rs[:, 0, 0]; rs[:, 1, 1] = rs[:, 0, 1] + BALL_AWAY
    rs[:, 1, 2] = B.ball_radius() - rng.uniform(*BALL_DEPTH, n)
    rs[:, 1, 6] = 1.0
    rs[:, 1, 7:9] = rng.uniform(-0.5, 0.5, (n, 2)) * scale
    rs[:, 1, 10:13] = rng.uniform(-3.0, 3.0, (n, 3)) * scale


def free_states(n, asset, seed=4):
    """env e aims at ground point e % 22 with the (e // 22)-th posture of the point's pool"""
    rng = np.random.default_rng(seed)
    pool = free_pool(asset)
    rs = np.zeros((n, 2, 13)); ds = np.zeros((n, 18, 2))
    aim = np.arange(n) % NPT
    for e in range(n):
        quat, q, z = pool[aim[e]]
        k = (e // NPT) % len(z)
        rs[e, 0, 3:7], ds[e, :, 0], rs[e, 0, 2] = quat[k], q[k], z[k]
    scale = np.where((np.arange(n) // NPT) % 4 == 3, SLOW, 1.0)[:, None]
    rs[:, 0, 7:10] = rng.uniform(-0.3, 0.3, (n, 3)) * scale
    rs[:, 0, 10:13] = rng.uniform(-1.0, 1.0, (n, 3)) * scale
    ds[:, :, 1] = rng.uniform(-1.0, 1.0, (n, 18)) * scale
    _ball_on_ground(rs, rng, scale)
    return dict(root_states=rs.astype(np.float32), dof_state=ds.astype(np.float32), aim=aim, slow=scale[:, 0] < 1.0)


def lying_states(n, asset, seed=5):
    rng = np.random.default_rng(seed)
    pool = lying_pool(asset)
    idx = lying_selection(pool, n, asset)
    rs = np.zeros((n, 2, 13)); ds = np.zeros((n, 18, 2))
    rs[:, 0, 3:7], ds[:, :, 0], rs[:, 0, 2] = pool["quat"][idx], pool["q"][idx], pool["z"][idx]
    rs[:, 0, 7:10] = rng.uniform(-0.3, 0.3, (n, 3)) * LYING_SPEED
    rs[:, 0, 10:13] = rng.uniform(-1.0, 1.0, (n, 3)) * LYING_SPEED
    ds[:, :, 1] = rng.uniform(-1.0, 1.0, (n, 18)) * LYING_SPEED
    _ball_on_ground(rs, rng, LYING_SPEED)
    st = dict(root_states=rs.astype(np.float32), dof_state=ds.astype(np.float32), side=pool["side"][idx])
    st["aim"] = heights(st, asset)[:, :NPT].argmin(1)   # the deepest point
    return st


def torso_ball_states(n, asset, seed=6):
    """lying on the front or back with a torso point under the plane; the ball through a point of the torso box's upward face (the
    face-point construction of ball_contact_ref.free_space_states), 0.5 - 10 mm deep, no other box touching it"""
    rng = np.random.default_rng(seed)
    pool = lying_pool(asset)
    cand = np.flatnonzero((pool["side"] < 2) & under_bodies(pool["under"], asset)[:, 0])
    assert len(cand) >= n, len(cand)
    T = tables(asset)
    R = B.ball_radius()
    box = B.box_table(asset)[-1]
    assert box["link"] == 0
    picked, centres = [], []
    for start in range(0, len(cand), n):
        idx = cand[start:start + n]
        m = len(idx)
        quat, q, z = pool["quat"][idx], pool["q"][idx], pool["z"][idx]
        E, r = link_frames(T, quat, q, np.float64)
        up = E[:, 0, 2, :]                                   # world z component of the torso's three axes
        axis = np.abs(up).argmax(1); sign = np.sign(up[np.arange(m), axis])
        p = rng.uniform(-0.8, 0.8, (m, 3)) * box["half"]
        p[np.arange(m), axis] = sign * box["half"][axis]
        normal = np.zeros((m, 3)); normal[np.arange(m), axis] = sign
        depth = rng.uniform(0.5e-3, 10e-3, m)
        local = box["center"] + p + normal * (R - depth)[:, None]
        bc = np.einsum("nij,nj->ni", E[:, 0], local)
        gap = P.ball_rows(T, E, r, bc, np.zeros((m, 3)), np.float64)[:, :, P.GAP]
        ok = (gap[:, -1] < -0.4e-3) & (gap[:, :-1] >= CLEAR).all(1)
        picked.extend(idx[ok].tolist()); centres.extend(bc[ok])
        if len(picked) >= n:
            break
    assert len(picked) >= n, len(picked)
    idx = np.array(picked[:n]); bc = np.array(centres[:n])
    rs = np.zeros((n, 2, 13)); ds = np.zeros((n, 18, 2))
    rs[:, 0, 3:7], ds[:, :, 0], rs[:, 0, 2] = pool["quat"][idx], pool["q"][idx], pool["z"][idx]
    rs[:, 0, 7:10] = rng.uniform(-0.3, 0.3, (n, 3)) * LYING_SPEED
    rs[:, 0, 10:13] = rng.uniform(-1.0, 1.0, (n, 3)) * LYING_SPEED
    ds[:, :, 1] = rng.uniform(-1.0, 1.0, (n, 18)) * LYING_SPEED
    rs[:, 1, 0:3] = rs[:, 0, 0:3] + bc
    rs[:, 1, 6] = 1.0
    rs[:, 1, 7:10] = rs[:, 0, 7:10] + rng.uniform(-0.1, 0.1, (n, 3))
    rs[:, 1, 10:13] = rng.uniform(-3.0, 3.0, (n, 3)) * LYING_SPEED
    st = dict(root_states=rs.astype(np.float32), dof_state=ds.astype(np.float32), side=pool["side"][idx])
    st["aim"] = heights(st, asset)[:, :NPT].argmin(1)
    return st


def lifted(states, keep):
    """a copy of `states` with the robot and the ball LIFT higher in every env that is not listed in `keep`; aim -1 there"""
    rs = states["root_states"].copy()
    away = np.ones(len(rs), bool); away[np.asarray(keep)] = False
    rs[away, :, 2] += np.float32(LIFT)
    return dict(states, root_states=rs, aim=np.where(away, -1, states["aim"]))


def case_states(scenario, asset, n):
    if scenario == "lying":
        return lying_states(n, asset)
    if scenario == "torso_ball":
        return torso_ball_states(n, asset)
    st = free_states(n, asset)
    if scenario == "sparse":
        return lifted(st, S.NEIGHBOUR_ENVS)
    assert scenario in ("free", "solo"), scenario
    return st


# ---------------------------------------------------------------------------------------------------------------- momentum
def robot_com(sim, n, asset):
    """(n, 3) the robot's centre of mass in the env frame, from the root and DOF state and the URDF masses (tests/centroidal_numpy.py)"""
    from tests import centroidal_numpy as CM
    from tests import dynamics_numpy as D
    root = sim.root_states.reshape(n, 2, 13)[:, 0].astype(np.float64)
    dof = sim.dof_state.reshape(n, 18, 2).astype(np.float64)
    links = D.model_of(asset)["links"]
    _, _, _, m, c, _ = CM._configuration(links, root[:, 3:7], dof[:, :, 0], np.ones((n, len(links))), np.float64)
    return root[:, 0:3] + sum(m[i][:, None] * c[i] for i in range(len(links))) / sum(m)[:, None]


def momentum_residual(before, after, com, point, cf, asset, dt):
    """(n, 2): largest component of [change of the robot's linear momentum - dt x the sum of its contact rows] (kg m/s) and of [change of
    its angular momentum about its centre of mass - dt x the moment of that sum, acting at `point` (n, 3), about the centre of mass `com`
    of the start state] (kg m^2/s).  The rows must hold the whole force (BEZ_FLAG_CF_WITH_FRICTION, one substep) of one point."""
    nb = B.ball_row(asset)
    f = np.asarray(cf, np.float64).reshape(len(com), -1, 3)[:, :nb].sum(1)
    lin = (after[0] - before[0]) - dt * f
    ang = (after[1] - before[1]) - dt * np.cross(point - com, f)
    return np.stack([np.abs(lin).max(1), np.abs(ang).max(1)], 1)


# ---------------------------------------------------------------------------------------------------------------- the oracle's side of a case
def reference(scenario, asset, n, substeps=2, dr=False, flags=0, contact=None, states=None, tag=None):
    """step_terms.reference of a ground case: states, per-env parameters, actions, the numpy terms of the start state, kept, both
    outputs, the momentum residuals.
    contact: ((BezSimConfig field, value), ...) set in the config of oracle and sim alike.  states / tag: another state set under the
    scenario's config (the planted slips)."""
    def cfg():
        c = S.step_cfg(n, asset, gravity=scenario in GRAVITY, substeps=substeps, flags=flags)
        for k, v in contact or ():
            setattr(c, k, v)
        return c

    def build(ref):
        ref.cfg = cfg
        ref.states = case_states(scenario, asset, n) if states is None else states
        ref.aim = ref.states["aim"]
        ref.params = S.dr_params(n, 8) if dr else None
        ref.actions = S.actions(n, 2)
        pair = S.oracle_pair(ref)
        rb = pair[0].rigid_body_states.reshape(n, -1, 13)
        ref.terms = terms(ref.states, asset, rb, cfg(), None if not dr else ref.params[abi.PARAM_FRICTION])
        ref.kept = kept(ref.terms)
        if scenario == "torso_ball":
            ref.depths = B.depths(rb, ref.states["root_states"][:, 1, 0:3], asset)
            ref.kept &= B.kept(ref.depths)
        ref.point = ref.states["root_states"][:, 0, 0:3].astype(np.float64) + points_rel(
            asset, ref.states["root_states"][:, 0, 3:7], ref.states["dof_state"][:, :, 0])[np.arange(n), np.maximum(ref.aim, 0)]
        before = [S.robot_momentum(o, n, asset) for o in pair]
        ref.com = robot_com(pair[0], n, asset)
        S.step_pair(ref, *pair)
        dt = float(cfg().dt)
        ref.res64, ref.res32 = (momentum_residual(b, S.robot_momentum(o, n, asset), ref.com, ref.point, out["cf"], asset, dt)
                                for b, o, out in zip(before, pair, (ref.out64, ref.out32)))
    return S.reference(("ground", scenario, asset, n, substeps, dr, flags, contact, tag), build,
                       scenario=scenario, asset=asset, n=n, substeps=substeps, dr=dr, flags=flags, contact=contact)


LAST, FRIC = abi.FLAG_CF_LAST_SUBSTEP, abi.FLAG_CF_WITH_FRICTION
# every oracle case of tests/test_gpu_ground_contact.py: (scenario, asset, n, substeps, dr, flags, contact)
CASES = ([("free", a, N, 2, dr, 0, None) for a in S.ASSETS for dr in (False, True)]
         + [("solo", a, N, 1, False, f, None) for a in ("default", "cleats") for f in (0, FRIC)]
         + [("lying", "default", N, s, False, 0, None) for s in (1, 2, 3, 4)] + [("lying", "default", N, 3, False, LAST | FRIC, None)]
         + [("lying", a, N, 2, False, 0, None) for a in ("cleats", "box")]
         + [("torso_ball", "default", 200, 2, False, 0, None), ("free", "default", N, 2, False, 0, PARAMS),
            ("free", "default", 200, 2, False, 0, None), ("sparse", "default", 200, 2, False, 0, None)])


def case_name(scenario, asset, n, substeps, dr, flags, contact):
    return "%s%s-s%d%s%s%s%s %s" % (scenario, "" if n == N else str(n), substeps, "-dr" if dr else "", "-fric" if flags & FRIC else "",
                                    "-last" if flags & LAST else "", "-params" if contact else "", asset)


def compare(case, ref, out, label, report=None, p99=True):
    """step_terms.compare, and per aimed point the worst contact-force error of its kept envs outside the outliers within the cf bar"""
    return S.compare(case, ref, out, label, report=report, p99=p99,
                     elements=lambda bars, bad: ((), S.aimed_cf_checks(ref, out, bars, bad, NPT, "point")))


def coverage_line(name, ref):
    """the case's own coverage: envs per aimed point, envs in which each point is active, regime counts over the kept envs"""
    aimed = np.bincount(ref.aim[ref.aim >= 0], minlength=NPT)
    act = ref.terms["active"][ref.kept][:, :NPT].sum(0)
    reg = regime_counts(ref.terms, ref.kept)
    return "%-36s aimed 0..21: %s  active 0..21: %s  ball active: %d  regimes: %s" % (
        name, " ".join(map(str, aimed)), " ".join(map(str, act)), ref.terms["active"][ref.kept][:, BALL].sum(),
        " ".join("%s=%d" % kv for kv in reg.items()))


# ---------------------------------------------------------------------------------------------------------------- planted slips
SLIPS = ("contact_cn", "plane_friction", "contact_ct", "contact_veps", "ball_kn", "ball_cn", "cf_last_substep", "forearm_rows_swapped",
         "head_into_torso", "torso_point_moved")
SLIP_POINT, SLIP_SHIFT = 9, 0.5e-3   # proximity_numpy's "ground_point" mutation: point 9's local z moved by 0.5 mm


def _scaled(contact, field, factor):
    return tuple((k, v * factor if k == field else v) for k, v in contact)


def planted(slip):
    """(ref, outputs): a case and the fp32 build's outputs of the same case with one thing made wrong -- on the oracle side only, no
    kernel is edited.
      contact_cn, plane_friction, contact_ct      free, 2 substeps: + 5 %, 1.0 -> 0.9, halved, in the config
      contact_veps, ball_kn, ball_cn              the params case: doubled, + 5 %, + 5 %, in the config
      cf_last_substep                             lying, 3 substeps: BEZ_FLAG_CF_LAST_SUBSTEP set where the mean is expected
      forearm_rows_swapped, head_into_torso       free: in the outputs' contact rows
      torso_point_moved                           free: torso point 9's local z moved by 0.5 mm -- the envs aimed at it step from a root
                                                  lifted by the height that shift has in the world"""
    assert slip in SLIPS
    d = abi.CONTACT_DEFAULTS
    free = ("free", "default", N)
    if slip in ("contact_cn", "plane_friction", "contact_ct"):
        wrong = {"contact_cn": 1.05 * d["contact_cn"], "plane_friction": 0.9, "contact_ct": 0.5 * d["contact_ct"]}[slip]
        return reference(*free), reference(*free, contact=((slip, wrong),)).out32
    if slip in ("contact_veps", "ball_kn", "ball_cn"):
        return reference(*free, contact=PARAMS), reference(*free, contact=_scaled(PARAMS, slip, 2.0 if slip == "contact_veps" else 1.05)).out32
    if slip == "cf_last_substep":
        return reference("lying", "default", N, substeps=3), reference("lying", "default", N, substeps=3, flags=LAST).out32
    ref = reference(*free)
    if slip == "torso_point_moved":
        st = ref.states
        E = B.quat_to_mat(st["root_states"][:, 0, 3:7])
        rs = st["root_states"].copy()
        envs = ref.aim == SLIP_POINT
        rs[envs, 0, 2] += (SLIP_SHIFT * E[envs, 2, 2]).astype(np.float32)
        return ref, reference(*free, states=dict(st, root_states=rs), tag=slip).out32
    out = {k: v.copy() for k, v in ref.out32.items()}
    cf = out["cf"].reshape(ref.n, -1, 3)
    pb = point_bodies("default")
    if slip == "forearm_rows_swapped":
        cf[:, [pb[20], pb[21]]] = cf[:, [pb[21], pb[20]]]
    else:
        cf[:, pb[8]] += cf[:, pb[16]]
    return ref, out
