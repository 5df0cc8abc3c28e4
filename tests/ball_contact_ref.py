"""Ball <-> box contact of the fused step: state generators that put the ball against every one of the eleven boxes, an independent
numpy sphere-box test, and the oracle's side of the cases of tests/test_ball_contact_cpu.py and tests/test_gpu_ball_contact.py (the
harness they share with the other step-term suites is tests/step_terms.py).

`depths` reads only the model JSON and the Isaac-visible rigid-body rows: it calls neither the oracle nor the kernels, so its choice of
the deepest box is evidence about both.  The generators use their own forward kinematics of the model JSON (checked against the
oracle's rigid-body rows in the CPU test)."""
import json
import os

import numpy as np

from tests import step_terms as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODEL = os.path.join(ROOT, "bez_isaacgym_amd", "model", "bez_model.json")
NBOX = 11
KEPT_MARGIN = 1e-4   # m: a deepest box that leads by less may be chosen either way by two roundings (DESIGN.md 6 "knife edges")
PARKED = (0.0, 3.0, 0.08)

_model = None


def model():
    global _model
    if _model is None:
        _model = json.load(open(MODEL))
    return _model


def asset_links(asset):
    """the link table of the asset (the cleats asset has its own link -> body map)"""
    m = model()
    return m["cleats"]["links"] if asset == "cleats" else m["links"]


def box_table(asset):
    """eleven boxes: link, body row, centre and half extents in the link frame; hip -> foot of the left leg, of the right leg, the torso"""
    m = model()
    links = asset_links(asset)
    boxes = [dict(b) for b in m["boxes"]]
    if asset == "box":
        boxes[-1] = dict(m["box_asset"]["torso_box"])
    assert len(boxes) == NBOX
    return [dict(link=int(b["link"]), body=int(links[b["link"]]["body"]), center=np.asarray(b["center"], np.float64),
                 half=np.asarray(b["half"], np.float64)) for b in boxes]


def ball_radius():
    return float(model()["ball"]["radius"])


def ball_row(asset):
    """row of the ball in the body tensors = number of robot bodies"""
    m = model()
    return int(m["cleats"]["num_bodies"] if asset == "cleats" else m["num_bodies"])


def owner_groups(asset):
    """which part of the wave kernels tests box b (bez_kernel_ws8.h cand_split): 0 = role 2 (upper leg boxes), 1 = roles 4 / 5 (lower leg
    boxes), 2 = the leg role's own foot box (assets without cleat records), 3 = role 3 (torso box)"""
    per_leg = (0, 0, 0, 1, 1) if asset == "cleats" else (0, 0, 1, 1, 2)
    return np.array(list(per_leg) * 2 + [3])


def quat_to_mat(q):
    """xyzw (..., 4) -> rotation body -> world (..., 3, 3)"""
    q = np.asarray(q, np.float64)
    x, y, z, w = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], -1),
                     np.stack([2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)], -1),
                     np.stack([2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], -1)], -2)


def depths(rb, ball_centre, asset):
    """(n, 11) fp64 sphere-box penetration depths (m; <= 0: no overlap) from the rigid-body rows rb (n, rows, 13) and the ball centre (n, 3):
    the link frame is the body row's position + quaternion; outside the box R - distance to the clamped centre, centre inside the box
    R + the smallest distance to a face."""
    rb = np.asarray(rb, np.float64)
    c = np.asarray(ball_centre, np.float64)
    R = ball_radius()
    out = np.empty((rb.shape[0], NBOX))
    for b, box in enumerate(box_table(asset)):
        row = rb[:, box["body"]]
        E = quat_to_mat(row[:, 3:7])
        ql = np.einsum("nji,nj->ni", E, c - row[:, 0:3]) - box["center"]
        cp = np.clip(ql, -box["half"], box["half"])
        dist = np.linalg.norm(ql - cp, axis=1)
        face = (box["half"] - np.abs(ql)).min(1)
        out[:, b] = np.where(face >= 0, R + face, R - dist)
    return out


def centre_inside(d):
    """envs whose ball centre lies inside some box"""
    return (d > ball_radius()).any(1)


def winner(d):
    """index of the deepest box, -1 where no box overlaps the ball"""
    w = d.argmax(1)
    return np.where(d.max(1) > 0, w, -1)


def runner_up(d):
    """index of the second-deepest box where its depth is positive, else -1"""
    order = np.argsort(-d, axis=1, kind="stable")
    second = order[:, 1]
    return np.where(d[np.arange(len(d)), second] > 0, second, -1)


def kept(d):
    """envs whose deepest candidate beats the second-deepest positive one by more than KEPT_MARGIN; an env with fewer than two overlapping
    boxes has nothing to decide between and is kept"""
    s = np.sort(d, axis=1)
    first, second = s[:, -1], s[:, -2]
    return (second <= 0) | (first - second > KEPT_MARGIN)


# ---------------------------------------------------------------------------------------------------------------- forward kinematics
def _rot_axis(axis, th):
    a = np.asarray(axis, np.float64)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(th)[:, None, None] * K + (1 - np.cos(th))[:, None, None] * (K @ K)


def link_frames(asset, root_pos, root_quat, q):
    """world rotation (n, L, 3, 3) and origin (n, L, 3) of every link from the model JSON's joint origins and axes"""
    links = asset_links(asset)
    n = len(q)
    E = np.empty((n, len(links), 3, 3)); r = np.empty((n, len(links), 3))
    E[:, 0] = quat_to_mat(root_quat); r[:, 0] = root_pos
    for i in range(1, len(links)):
        p = links[i]["parent"]
        r[:, i] = r[:, p] + np.einsum("nij,j->ni", E[:, p], np.asarray(links[i]["xyz"], np.float64))
        E[:, i] = E[:, p] @ _rot_axis(links[i]["axis"], np.asarray(q[:, i - 1], np.float64))
    return E, r


# ---------------------------------------------------------------------------------------------------------------- generators
def free_space_states(n, asset, seed):
    """Zero gravity, robot at z = 1 with a random torso attitude, moving; env e has the ball 0.5 - 10 mm deep in box e % 11 through a
    uniformly chosen face point.  Returns root_states (n, 2, 13) and dof_state (n, 18, 2), fp32, Isaac layouts."""
    rng = np.random.default_rng(seed)
    R = ball_radius()
    dflt = np.asarray(model()["dof_default"], np.float64)
    rs = np.zeros((n, 2, 13)); ds = np.zeros((n, 18, 2))
    quat = rng.normal(size=(n, 4)); quat /= np.linalg.norm(quat, axis=1, keepdims=True)
    rs[:, 0, 2] = 1.0
    rs[:, 0, 3:7] = quat
    rs[:, 0, 7:10] = rng.uniform(-0.3, 0.3, (n, 3))
    rs[:, 0, 10:13] = rng.uniform(-1.0, 1.0, (n, 3))
    ds[:, :, 0] = dflt + rng.uniform(-0.3, 0.3, (n, 18))
    ds[:, :, 1] = rng.uniform(-1.0, 1.0, (n, 18))
    # the kernels and the oracle see the fp32 state: aim from it
    rs32, ds32 = rs.astype(np.float32), ds.astype(np.float32)
    E, r = link_frames(asset, rs32[:, 0, 0:3], rs32[:, 0, 3:7], ds32[:, :, 0])
    boxes = box_table(asset)
    env = np.arange(n)
    aim = env % NBOX
    link = np.array([boxes[b]["link"] for b in aim])
    centre = np.stack([boxes[b]["center"] for b in aim]); half = np.stack([boxes[b]["half"] for b in aim])
    face_axis = rng.integers(0, 3, n); face_sign = rng.choice([-1.0, 1.0], n)
    p = rng.uniform(-1.0, 1.0, (n, 3)) * half
    p[env, face_axis] = face_sign * half[env, face_axis]
    normal = np.zeros((n, 3)); normal[env, face_axis] = face_sign
    depth = rng.uniform(0.5e-3, 10e-3, n)
    local = centre + p + normal * (R - depth)[:, None]
    rs[:, 1, 0:3] = r[env, link] + np.einsum("nij,nj->ni", E[env, link], local)
    rs[:, 1, 6] = 1.0
    rs[:, 1, 7:10] = rs[:, 0, 7:10] + rng.uniform(-0.5, 0.5, (n, 3))
    rs[:, 1, 10:13] = rng.uniform(-3.0, 3.0, (n, 3))
    return dict(root_states=rs.astype(np.float32), dof_state=ds.astype(np.float32), aim=aim)


def kick_stance_states(n, asset, seed, reset_root=None, reset_dof=None):
    """The reset state (as a freshly created sim of step_terms.step_cfg(n, asset) reports it, bit for bit the same from the oracle and the kernels:
    standing on the ground under default gravity) with the ball resting on the ground, at most 2 mm into it, on a circle of radius
    0.06 - 0.125 m around the left foot (even envs) or the right foot (odd envs), rolling at up to 0.5 m/s with up to 3 rad/s of spin."""
    rng = np.random.default_rng(seed)
    R = ball_radius()
    if reset_root is None:
        from oracle.bez_oracle import Oracle
        fresh = Oracle(S.step_cfg(n, asset))
        reset_root, reset_dof = fresh.root_states, fresh.dof_state
    rs = np.asarray(reset_root, np.float64).reshape(n, 2, 13).copy()
    ds = np.asarray(reset_dof, np.float64).reshape(n, 18, 2).copy()
    _, r = link_frames(asset, rs[:, 0, 0:3], rs[:, 0, 3:7], ds[:, :, 0])
    boxes = box_table(asset)
    env = np.arange(n)
    foot = r[env, np.where(env % 2 == 0, boxes[4]["link"], boxes[9]["link"])]
    rad = rng.uniform(0.06, 0.125, n); phi = rng.uniform(0.0, 2.0 * np.pi, n)
    rs[:, 1, :] = 0.0
    rs[:, 1, 0] = foot[:, 0] + rad * np.cos(phi)
    rs[:, 1, 1] = foot[:, 1] + rad * np.sin(phi)
    rs[:, 1, 2] = R - rng.uniform(0.0, 2e-3, n)
    rs[:, 1, 6] = 1.0
    rs[:, 1, 7:9] = rng.uniform(-0.5, 0.5, (n, 2))
    rs[:, 1, 10:13] = rng.uniform(-3.0, 3.0, (n, 3))
    return dict(root_states=rs.astype(np.float32), dof_state=ds.astype(np.float32))


def park_ball(states, keep):
    """a copy of `states` with the ball at rest at PARKED in every env that is not listed in `keep`"""
    rs = states["root_states"].copy()
    away = np.ones(len(rs), bool); away[np.asarray(keep)] = False
    rs[away, 1, :] = 0.0
    rs[away, 1, 0:3] = PARKED
    rs[away, 1, 6] = 1.0
    return dict(states, root_states=rs)


# ---------------------------------------------------------------------------------------------------------------- rows and momentum
def loaded_rows(cf, asset, tol=0.0):
    """(n, robot bodies) bool: robot rows of the contact-force tensor (n * rows, 3) that carry a force"""
    nb = ball_row(asset)
    rows = np.asarray(cf).reshape(-1, nb + 1, 3)
    return np.abs(rows[:, :nb]).max(2) > tol


def winner_body(d, asset):
    """body row of the deepest box, -1 where nothing overlaps"""
    bodies = np.array([b["body"] for b in box_table(asset)])
    w = winner(d)
    return np.where(w >= 0, bodies[np.maximum(w, 0)], -1)


def robot_ball_momentum(sim, n, asset):
    """linear momentum of the robot (step_terms.robot_momentum) and of the ball, from the rigid-body rows"""
    rb = sim.rigid_body_states.reshape(n, -1, 13).astype(np.float64)
    return S.robot_momentum(sim, n, asset)[0], float(model()["ball"]["mass"]) * rb[:, ball_row(asset), 7:10]


def momentum_change(before, after):
    """(n,) largest component of the change of robot + ball linear momentum (kg m/s)"""
    return np.abs((after[0] + after[1]) - (before[0] + before[1])).max(1)


# ---------------------------------------------------------------------------------------------------------------- the oracle's side of a case
def case_states(scenario, asset, n):
    """the states of a scenario: "free" (free_space_states), "kick" (kick_stance_states), "sparse" (free space, the ball parked away
    from the robot in every env but step_terms.NEIGHBOUR_ENVS)"""
    if scenario == "kick":
        return kick_stance_states(n, asset, 3)
    st = free_space_states(n, asset, 4)
    return park_ball(st, S.NEIGHBOUR_ENVS) if scenario == "sparse" else st


def reference(scenario, asset, n, substeps=2, dr=False, flags=0):
    """step_terms.reference of a ball case: states, per-env parameters, actions, the numpy depths of the start state, kept, both
    outputs, the momentum change."""
    def build(ref):
        ref.cfg = lambda: S.step_cfg(n, asset, gravity=(scenario == "kick"), substeps=substeps, flags=flags)
        ref.states = case_states(scenario, asset, n)
        ref.params = S.dr_params(n, 8) if dr else None
        ref.actions = S.actions(n, 2)
        pair = S.oracle_pair(ref)
        ref.depths = depths(pair[0].rigid_body_states.reshape(n, -1, 13), ref.states["root_states"][:, 1, 0:3], asset)
        ref.kept = kept(ref.depths)
        before = [robot_ball_momentum(o, n, asset) for o in pair]
        S.step_pair(ref, *pair)
        ref.dp64, ref.dp32 = (momentum_change(b, robot_ball_momentum(o, n, asset)) for b, o in zip(before, pair))
    return S.reference(("ball", scenario, asset, n, substeps, dr, flags), build,
                       scenario=scenario, asset=asset, n=n, substeps=substeps, dr=dr, flags=flags)
