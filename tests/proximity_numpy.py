"""Reference for bez_sim_proximity (include/bez_sim.h "Proximity"): the ground points' positions, the signed distance of the ball to the
eleven boxes and of the 28 left-leg x right-leg capsule pairs, from bez_model.json alone.  Test-only.

  proximity_ref   its own forward kinematics (Rodrigues rotations of the model's axes; the kernels go through link_kinematics' column
                  rotations) relative to the root origin, root_pos joining in the last addition of every env-coordinate output; the
                  sphere-box test written from the definition; the segment-segment distance by an algorithm that shares nothing with the
                  kernels' (segment_closest: the unconstrained s, the t it implies, clamps): the interior stationary point where it lies
                  inside both segments, and the four end-point-to-segment distances, the smallest of the five.
  dtype=np.float64 is the reference; the same code in np.float32 is the yardstick of fp32 rounding for the GPU bars (yardstick_error).
  The root quaternion is used as it is given (as the kernels use it).
  Assets: "default", "cleats", "box", "box_cleats" (the asset whose right ankle's joint origin is the model's
  box_asset.cleats_right_ankle_xyz).
  contact_states  the seeded state set that meets every pair overlapping and apart, every box through a face, an edge, a corner and with
                  the ball's centre inside, and every ground point on both sides of the plane."""
import json
import os

import numpy as np

from tests.limb_ik_numpy import quat_to_mat

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODEL = json.load(open(os.path.join(ROOT, "bez_isaacgym_amd", "model", "bez_model.json")))
ASSETS = ("default", "cleats", "box", "box_cleats")
NPT, NBOX, NCAP, NPAIR, WORDS = 22, 11, 12, 28, 8
GAP, NORMAL, POINT = 0, slice(1, 4), slice(4, 7)
MEET2 = 1e-12          # squared axis distance at and below which a pair has no direction (the step applies no force there)
PAIR_MIN_DIST = 2e-3   # m: below this axis distance, and
PAIR_MIN_SIN2 = 1e-2   # below this sin^2 of the angle between the axes, a pair's normal and point are not compared
BALL_MARGIN = 1e-4     # m: within this of the box surface, or of a tie between the two nearest faces, a ball row's normal and point are not compared
MUTATIONS = ("capsule_radius", "box_half_extent", "ground_point", "normal_reversed")
BLOCKS = ("ground_xy", "ground_z", "ball_gap", "ball_normal", "ball_point", "pair_gap", "pair_normal", "pair_point")
MODES = ("face", "edge", "corner", "inside")


def tables(asset, mutate=None):
    """the asset's geometry: links, ground points (22, 3) with their links, boxes, capsules, pairs, ball radius -- all fp64"""
    assert asset in ASSETS and (mutate is None or mutate in MUTATIONS)
    m = MODEL
    cleats, box = "cleats" in asset, "box" in asset
    links = [dict(parent=int(L["parent"]), axis=np.asarray(L["axis"], np.float64), xyz=np.asarray(L["xyz"], np.float64), name=L["name"]) for L in m["links"]]
    if cleats and box:
        for L in links:
            if L["name"] == "/right_ankle":
                L["xyz"] = np.asarray(m["box_asset"]["cleats_right_ankle_xyz"], np.float64)
    feet = (m["cleats"] if cleats else m)["ground_points"]
    upper = (m["box_asset"] if box else m)["ground_points"]
    pts = [feet[i] if i < 8 else upper[i] for i in range(NPT)]
    assert [p["link"] for p in pts] == [p["link"] for p in m["ground_points"]]
    boxes = [dict(b) for b in m["boxes"]]
    if box:
        boxes[-1] = dict(m["box_asset"]["torso_box"])
    T = dict(links=links, pt_link=np.array([p["link"] for p in pts]), pt_pos=np.array([p["p"] for p in pts], np.float64),
             box_link=np.array([b["link"] for b in boxes]), box_center=np.array([b["center"] for b in boxes], np.float64),
             box_half=np.array([b["half"] for b in boxes], np.float64),
             cap_link=np.array([c["link"] for c in m["capsules"]]), cap_p0=np.array([c["p0"] for c in m["capsules"]], np.float64),
             cap_p1=np.array([c["p1"] for c in m["capsules"]], np.float64), cap_r=np.array([c["r"] for c in m["capsules"]], np.float64),
             pairs=np.array(m["capsule_pairs"]), R=float(m["ball"]["radius"]))
    assert T["pt_pos"].shape == (NPT, 3) and len(boxes) == NBOX and len(T["cap_r"]) == NCAP and T["pairs"].shape == (NPAIR, 2)
    if mutate == "capsule_radius":
        T["cap_r"][2] *= 1.01
    elif mutate == "box_half_extent":
        T["box_half"][3, 0] += 1e-3
    elif mutate == "ground_point":
        T["pt_pos"][9, 2] += 0.5e-3
    return T


def _mv(M, v):
    return np.einsum("...ij,...j->...i", M, v)


def _mtv(M, v):
    return np.einsum("...ji,...j->...i", M, v)


def link_frames(T, root_quat, q, f=np.float64):
    """rotation (n, L, 3, 3) and origin (n, L, 3) of every link in world axes RELATIVE TO THE ROOT ORIGIN, in dtype f"""
    links = T["links"]
    q = np.asarray(q).astype(f)
    n = q.shape[0]
    E = np.empty((n, len(links), 3, 3), f); r = np.zeros((n, len(links), 3), f)
    E[:, 0] = quat_to_mat(np.asarray(root_quat).astype(f), f)
    eye = np.eye(3, dtype=f)
    for i in range(1, len(links)):
        L = links[i]
        p = L["parent"]
        r[:, i] = r[:, p] + _mv(E[:, p], L["xyz"].astype(f))
        a = L["axis"].astype(f)
        K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]], f)
        th = q[:, i - 1][:, None, None]
        E[:, i] = E[:, p] @ (eye + np.sin(th) * K + (f(1) - np.cos(th)) * (K @ K))
    assert E.dtype == f and r.dtype == f
    return E, r


def _dot(a, b):
    return (a * b).sum(-1)


def _point_segment(x, p, d, dd, f):
    """parameter in [0, 1] of the point of the segment p + u d closest to x"""
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.clip(_dot(x - p, d) / dd, f(0), f(1))


def segment_closest(p1, q1, p2, q2, f=np.float64):
    """closest points (c1 on p1-q1, c2 on p2-q2) of two segments, (..., 3) each: the smallest of five candidates -- the stationary
    point of the squared distance over the two lines where it lies inside both segments, and each end point against the other segment.
    Returns (c1, c2, squared distance)."""
    d1, d2, r = q1 - p1, q2 - p2, p1 - p2
    a, e, b, c, g = _dot(d1, d1), _dot(d2, d2), _dot(d1, d2), _dot(d1, r), _dot(d2, r)
    den = a * e - b * b
    with np.errstate(invalid="ignore", divide="ignore"):
        s0 = (b * g - c * e) / den
        t0 = (a * g - b * c) / den
    ok = (den > f(1e-9) * a * e) & (s0 >= 0) & (s0 <= 1) & (t0 >= 0) & (t0 <= 1)
    zero, one = np.zeros_like(a), np.ones_like(a)
    cand = [(np.where(ok, s0, zero), np.where(ok, t0, zero), ok),
            (zero, _point_segment(p1, p2, d2, e, f), None), (one, _point_segment(q1, p2, d2, e, f), None),
            (_point_segment(p2, p1, d1, a, f), zero, None), (_point_segment(q2, p1, d1, a, f), one, None)]
    best = None
    for s, t, valid in cand:
        c1, c2 = p1 + s[..., None] * d1, p2 + t[..., None] * d2
        dd = _dot(c1 - c2, c1 - c2)
        if valid is not None:
            dd = np.where(valid, dd, f(np.inf))
        if best is None:
            best = [c1, c2, dd]
        else:
            take = dd < best[2]
            best = [np.where(take[..., None], c1, best[0]), np.where(take[..., None], c2, best[1]), np.where(take, dd, best[2])]
    nan = ~np.isfinite(a + e + b + c + g)
    best[2] = np.where(nan, f(np.nan), best[2])
    return best[0], best[1], best[2]


def capsule_axes(T, E, r, f):
    """end points (n, 12, 3) x 2 of the capsule axes relative to the root origin"""
    l = T["cap_link"]
    return r[:, l] + _mv(E[:, l], T["cap_p0"].astype(f)), r[:, l] + _mv(E[:, l], T["cap_p1"].astype(f))


def ball_rows(T, E, r, bc, root_pos, f):
    """(n, 11, 8): [gap, normal, point, 0] of the sphere with centre bc (relative to the root origin) against every box"""
    n = bc.shape[0]
    R = f(T["R"])
    l = T["box_link"]
    El, rl = E[:, l], r[:, l]
    cl, he = T["box_center"].astype(f), T["box_half"].astype(f)
    ql = _mtv(El, bc[:, None, :] - rl) - cl
    with np.errstate(invalid="ignore"):
        cp = np.minimum(np.maximum(ql, -he), he)
        inside = (cp == ql).all(-1)
        dlt = ql - cp
        dist = np.sqrt(_dot(dlt, dlt))
        with np.errstate(divide="ignore"):
            n_out = dlt / dist[..., None]
        face = he - np.abs(ql)
        ax = np.argmin(face, axis=-1)                      # the first of x, y, z on ties, as the step
        md = np.take_along_axis(face, ax[..., None], -1)[..., 0]
        sgn = np.where(np.take_along_axis(ql, ax[..., None], -1)[..., 0] >= 0, f(1), f(-1))
    n_in = np.zeros_like(ql)
    np.put_along_axis(n_in, ax[..., None], sgn[..., None], -1)
    cp_in = cp.copy()
    np.put_along_axis(cp_in, ax[..., None], (sgn * np.take_along_axis(np.broadcast_to(he, ql.shape), ax[..., None], -1)[..., 0])[..., None], -1)
    gap = np.where(inside, -(R + md), dist - R)
    nl = np.where(inside[..., None], n_in, n_out)
    cpl = np.where(inside[..., None], cp_in, cp)
    out = np.zeros((n, NBOX, WORDS), f)
    out[:, :, GAP] = gap
    out[:, :, NORMAL] = _mv(El, nl)
    out[:, :, POINT] = root_pos[:, None, :] + (rl + _mv(El, cpl + cl))
    return out


def pair_rows(T, c0, c1, root_pos, f, reverse=None):
    """(n, 28, 8): [gap, normal b -> a, point cb + n (rb + gap / 2), 0] of every capsule pair"""
    n = c0.shape[0]
    ia, ib = T["pairs"][:, 0], T["pairs"][:, 1]
    ra, rb = T["cap_r"].astype(f)[ia], T["cap_r"].astype(f)[ib]
    ca, cb, d2 = segment_closest(c0[:, ia], c1[:, ia], c0[:, ib], c1[:, ib], f)
    with np.errstate(invalid="ignore", divide="ignore"):
        meet = d2 <= f(MEET2)
        dist = np.sqrt(d2)
        nrm = np.where(meet[..., None], f(0), (ca - cb) / dist[..., None])
        gap = np.where(meet, -(ra + rb), dist - (ra + rb))
        pt = np.where(meet[..., None], cb, cb + nrm * (rb + f(0.5) * gap)[..., None])
    if reverse is not None:
        nrm[:, reverse] = -nrm[:, reverse]
    out = np.zeros((n, NPAIR, WORDS), f)
    out[:, :, GAP] = gap
    out[:, :, NORMAL] = nrm
    out[:, :, POINT] = root_pos[:, None, :] + pt
    return out


def proximity_ref(asset, root, q, ball_pos, dtype=np.float64, mutate=None):
    """root (n, 13) or (n, 7), q (n, 18) or dof (n, 18, 2), ball_pos (n, 3): fp32 inputs as the sim holds them ->
    dict(ground (n, 23, 3), ball (n, 11, 8), pairs (n, 28, 8)) in `dtype`.  mutate: one of MUTATIONS, the slips the sensitivity check plants."""
    f = dtype
    T = tables(asset, mutate)
    root = np.asarray(root).astype(f)
    q = np.asarray(q)
    q = (q[:, :, 0] if q.ndim == 3 else q).astype(f)
    ball_pos = np.asarray(ball_pos).astype(f)
    n = root.shape[0]
    root_pos = root[:, 0:3]
    E, r = link_frames(T, root[:, 3:7], q, f)
    ground = np.zeros((n, NPT + 1, 3), f)
    l = T["pt_link"]
    ground[:, :NPT] = root_pos[:, None, :] + (r[:, l] + _mv(E[:, l], T["pt_pos"].astype(f)))
    ground[:, NPT] = ball_pos
    ground[:, NPT, 2] = ball_pos[:, 2] - f(T["R"])
    c0, c1 = capsule_axes(T, E, r, f)
    out = dict(ground=ground, ball=ball_rows(T, E, r, ball_pos - root_pos, root_pos, f),
               pairs=pair_rows(T, c0, c1, root_pos, f, reverse=10 if mutate == "normal_reversed" else None))
    assert all(v.dtype == f for v in out.values())
    return out


def conditioning(asset, root, q, ball_pos):
    """what the comparison of normals and points needs to know, in fp64: pair_ok (n, 28) -- the axis distance is >= PAIR_MIN_DIST and
    sin^2 of the angle between the axes >= PAIR_MIN_SIN2 (parallel legs leave the closest points non-unique); ball_ok (n, 11) -- the
    centre is farther than BALL_MARGIN from the box surface and, inside, the two smallest face distances differ by more than
    BALL_MARGIN; height (n, 22) of the ground points; ball_mode (n, 11): how many coordinates are clamped (1 face, 2 edge, 3 corner,
    0 centre inside)"""
    f = np.float64
    T = tables(asset)
    root = np.asarray(root).astype(f)
    q = np.asarray(q)
    q = (q[:, :, 0] if q.ndim == 3 else q).astype(f)
    bc = np.asarray(ball_pos).astype(f) - root[:, 0:3]
    E, r = link_frames(T, root[:, 3:7], q, f)
    c0, c1 = capsule_axes(T, E, r, f)
    ia, ib = T["pairs"][:, 0], T["pairs"][:, 1]
    d1, d2 = c1[:, ia] - c0[:, ia], c1[:, ib] - c0[:, ib]
    _, _, dd = segment_closest(c0[:, ia], c1[:, ia], c0[:, ib], c1[:, ib], f)
    cr = np.cross(d1, d2)
    sin2 = _dot(cr, cr) / (_dot(d1, d1) * _dot(d2, d2))
    with np.errstate(invalid="ignore"):
        pair_ok = (np.sqrt(dd) >= PAIR_MIN_DIST) & (sin2 >= PAIR_MIN_SIN2)
    l = T["box_link"]
    ql = _mtv(E[:, l], bc[:, None, :] - r[:, l]) - T["box_center"]
    he = T["box_half"]
    cp = np.clip(ql, -he, he)
    inside = (cp == ql).all(-1)
    dist = np.linalg.norm(ql - cp, axis=-1)
    face = np.sort(he - np.abs(ql), axis=-1)
    ball_ok = np.where(inside, (face[..., 0] > BALL_MARGIN) & (face[..., 1] - face[..., 0] > BALL_MARGIN), dist > BALL_MARGIN)
    mode = (cp != ql).sum(-1)
    lp = T["pt_link"]
    height = root[:, None, 2] + (r[:, lp] + _mv(E[:, lp], T["pt_pos"]))[..., 2]
    return dict(pair_ok=pair_ok, ball_ok=ball_ok, height=height, ball_mode=mode, pair_dist=np.sqrt(dd), pair_sin2=sin2)


def block_slices():
    """{block name: (which output, index)}"""
    a = slice(None)
    return {"ground_xy": ("ground", (a, a, slice(0, 2))), "ground_z": ("ground", (a, a, 2)),
            "ball_gap": ("ball", (a, a, GAP)), "ball_normal": ("ball", (a, a, NORMAL)), "ball_point": ("ball", (a, a, POINT)),
            "pair_gap": ("pairs", (a, a, GAP)), "pair_normal": ("pairs", (a, a, NORMAL)), "pair_point": ("pairs", (a, a, POINT))}


def compared(cond):
    """{block: None (every row of every env: the gaps and the ground rows) or the (n, rows) mask of the well-conditioned rows (normals
    and points)}"""
    return {"ground_xy": None, "ground_z": None, "ball_gap": None, "pair_gap": None, "ball_normal": cond["ball_ok"], "ball_point": cond["ball_ok"],
            "pair_normal": cond["pair_ok"], "pair_point": cond["pair_ok"]}


def block_errors(got, ref, cond, n=None):
    """{block: worst |got - ref| over what is compared, on the first n envs}; a non-finite difference counts as inf"""
    out = {}
    keep = compared(cond)
    for name, (w, ix) in block_slices().items():
        g, r = np.asarray(got[w], np.float64)[:n][ix], np.asarray(ref[w], np.float64)[:n][ix]
        with np.errstate(invalid="ignore"):
            err = np.abs(g - r)
        err = np.where(np.isfinite(err), err, np.inf)
        if keep[name] is not None:
            k = keep[name][:n]
            err = np.where(k[..., None] if err.ndim == 3 else k, err, 0.0)
        out[name] = float(err.max())
    return out


def yardstick_error(ref64, asset, root, q, ball_pos, cond):
    """{block: worst absolute error against ref64 of proximity_ref evaluated in np.float32 on the same inputs, over what is compared}"""
    return block_errors(proximity_ref(asset, root, q, ball_pos, dtype=np.float32), ref64, cond)


# ---------------------------------------------------------------------------------------------------------------- the contact state set
def contact_states(n, asset, seed=0):
    """fp32 (root (n, 13), dof (n, 18, 2), ball (n, 13)) and the plan (aim box, mode, aimed ground point) of every env:
      legs     env e aims at capsule pair e % 28, overlapping (even e // 28) or apart (odd): the leg joints are drawn, without regard
               to their limits (the call has none), until the pair's gap has the wanted sign with 2 - 15 mm to spare;
      ball     against box e % 11 in mode (e // 11) % 4: through a face, an edge, a corner (the centre outside by 0.3 - 1.2 R, so
               overlapping and apart both occur) or with the centre inside, at least 5 BALL_MARGIN from every tie;
      ground   root_pos.z puts ground point e % 22 at 1 - 40 mm above (even e // 22) or below (odd) the plane; roots up to 100 m out."""
    rng = np.random.default_rng(seed)
    T = tables(asset)
    f = np.float64
    dflt = np.asarray(MODEL["dof_default"], f)
    root = np.zeros((n, 13)); dof = np.zeros((n, 18, 2)); ball = np.zeros((n, 13))
    quat = rng.normal(size=(n, 4)); quat /= np.linalg.norm(quat, axis=1, keepdims=True)
    root[:, 3:7] = quat
    root[:, 0:2] = rng.uniform(-100, 100, (n, 2))
    root[:, 7:13] = rng.uniform(-1, 1, (n, 6))
    dof[:, :, 1] = rng.uniform(-5, 5, (n, 18))
    q = dflt + rng.uniform(-0.5, 0.5, (n, 18))
    legs = list(range(4, 10)) + list(range(12, 18))
    ia, ib = T["pairs"][:, 0], T["pairs"][:, 1]
    rs = T["cap_r"][ia] + T["cap_r"][ib]
    want_pair = np.arange(n) % NPAIR
    want_overlap = (np.arange(n) // NPAIR) % 2 == 0
    todo = np.ones(n, bool)
    for _ in range(4000):
        if not todo.any():
            break
        k = int(todo.sum())
        trial = q[todo].copy()
        trial[:, legs] = rng.uniform(-2.0, 2.0, (k, 12))
        E, r = link_frames(T, quat[todo].astype(np.float32), trial.astype(np.float32), f)
        c0, c1 = capsule_axes(T, E, r, f)
        p = want_pair[todo]
        _, _, dd = segment_closest(c0[np.arange(k), ia[p]], c1[np.arange(k), ia[p]], c0[np.arange(k), ib[p]], c1[np.arange(k), ib[p]], f)
        gap = np.sqrt(dd) - rs[p]
        good = np.where(want_overlap[todo], (gap < -2e-3) & (gap > -15e-3), (gap > 2e-3) & (gap < 15e-3))
        idx = np.flatnonzero(todo)[good]
        q[idx] = trial[good]
        todo[idx] = False
    assert not todo.any(), "no leg posture found for pairs %s" % sorted(set(want_pair[todo]))
    dof[:, :, 0] = q
    root32, dof32 = root.astype(np.float32), dof.astype(np.float32)
    E, r = link_frames(T, root32[:, 3:7], dof32[:, :, 0], f)
    # the ground: the aimed point's height decides root_pos.z
    env = np.arange(n)
    aim_pt = env % NPT
    lp = T["pt_link"][aim_pt]
    zrel = (r[env, lp] + _mv(E[env, lp], T["pt_pos"][aim_pt]))[:, 2]
    h = rng.uniform(1e-3, 40e-3, n) * np.where((env // NPT) % 2 == 0, 1.0, -1.0)
    root[:, 2] = h - zrel
    root32 = root.astype(np.float32)
    # the ball: placed in the aimed box's frame
    aim_box = env % NBOX
    mode = (env // NBOX) % 4
    lb = T["box_link"][aim_box]
    he, cl = T["box_half"][aim_box], T["box_center"][aim_box]
    local = np.zeros((n, 3))
    for e in range(n):
        m = 5 * BALL_MARGIN
        if mode[e] == 3:                                     # centre inside, the nearest face ahead of the next by >= 5 margins
            while True:
                x = rng.uniform(-1, 1, 3) * (he[e] - m)
                face = np.sort(he[e] - np.abs(x))
                if face[0] > m and face[1] - face[0] > m:
                    break
            local[e] = x
        else:
            nclamp = mode[e] + 1
            axes = rng.permutation(3)[:nclamp]
            x = rng.uniform(-1, 1, 3) * (he[e] - m)
            d = rng.normal(size=nclamp); d = np.abs(d) / np.linalg.norm(d)
            d = np.maximum(d, 0.15); d /= np.linalg.norm(d)   # every clamped coordinate clearly outside
            out = rng.uniform(0.3, 1.2) * T["R"]
            sg = rng.choice([-1.0, 1.0], nclamp)
            x[axes] = sg * (he[e, axes] + out * d)
            local[e] = x
    centre = root32[:, 0:3].astype(f) + r[env, lb] + _mv(E[env, lb], cl + local)
    ball[:, 0:3] = centre
    ball[:, 6] = 1.0
    ball[:, 7:13] = rng.uniform(-2, 2, (n, 6))
    return root32, dof32, ball.astype(np.float32), dict(pair=want_pair, overlap=want_overlap, box=aim_box, mode=mode, point=aim_pt)
