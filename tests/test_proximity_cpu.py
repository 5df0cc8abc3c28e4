"""CPU: the fp64 reference of bez_sim_proximity (tests/proximity_numpy.py) against independent implementations, and the coverage of the
state sets that tests/test_gpu_proximity.py hands to the kernel.

  ball gaps     equal -tests/ball_contact_ref.depths (the sphere-box test the step kernels are held to, which works from rigid-body rows)
  pair gaps     bounded by a dense sampling of both axis segments: the sampled minimum is >= the reference and within the grid's reach
  ground rows   the rigid-body rows' pose applied to the point offsets
  names         the abi tables against the model JSON
  coverage      every pair overlapping and apart, every box through a face, an edge, a corner and with the centre inside, every ground
                point above and below the plane; the left-out shares of the normals' comparison under their caps"""
import numpy as np
import pytest

from bez_isaacgym_amd import abi
from tests import ball_contact_ref as BC
from tests import proximity_numpy as P
from tests.state_sets import ball_states, generate_states

N = 300
PAIR_CAP, BALL_CAP = 0.25, 0.05


@pytest.fixture(scope="module")
def generated():
    root, dof, _ = generate_states(N)
    return root, dof, ball_states(N)


@pytest.fixture(scope="module")
def contact():
    return {asset: P.contact_states(N, asset, seed=7) for asset in P.ASSETS}


def _rigid_body_rows(asset, root, dof):
    """(n, bodies, 7) fp64 [position, quaternion xyzw] of the asset's bodies from the reference's own link frames"""
    from tests.limb_ik_numpy import mat_to_quat
    T = P.tables(asset)
    m = P.MODEL["cleats"] if "cleats" in asset else P.MODEL
    E, r = P.link_frames(T, root[:, 3:7], dof[:, :, 0])
    link = np.asarray(m["body_link"])
    off = np.asarray(m["body_offset"], np.float64)
    pos = root[:, None, 0:3].astype(np.float64) + r[:, link] + np.einsum("nbij,bj->nbi", E[:, link], off)
    quat = np.stack([mat_to_quat(E[:, l], np.float64) for l in link], axis=1)
    return np.concatenate([pos, quat], axis=2)


@pytest.mark.parametrize("asset", ["default", "cleats", "box"])
def test_ball_gaps_are_minus_the_depths_of_ball_contact_ref(asset):
    """free_space_states (the ball 0.5 - 10 mm into every box in turn) and kick_stance_states (the ball on the ground beside a foot): the
    reference's gaps against an implementation that shares no code with it and reads rigid-body rows"""
    sets = {"free": BC.free_space_states(N, asset, 4)}
    try:
        sets["kick"] = BC.kick_stance_states(64, asset, 3)
    except (ImportError, OSError) as e:   # the oracle's library is built on first use
        pytest.fail("the oracle is needed for the reset state: %r" % (e,))
    for name, st in sets.items():
        root, dof, ball = st["root_states"][:, 0].astype(np.float64), st["dof_state"], st["root_states"][:, 1]
        root[:, 3:7] /= np.linalg.norm(root[:, 3:7], axis=1, keepdims=True)   # (body rows carry unit quaternions; the reference takes the root's as given)
        ref = P.proximity_ref(asset, root, dof, ball[:, 0:3])
        d = BC.depths(_rigid_body_rows(asset, root, dof), ball[:, 0:3], asset)
        assert np.abs(ref["ball"][:, :, P.GAP] + d).max() < 1e-12, (name, np.abs(ref["ball"][:, :, P.GAP] + d).max())
        if name == "free":
            assert (d.max(axis=1) > 4e-4).all()
        # the normal is the gradient of the gap, the point lies on the box, the ball's centre is point + normal (gap + R) when outside
        outside = ref["ball"][:, :, P.GAP] > -BC.ball_radius()
        centre = ref["ball"][:, :, P.POINT] + ref["ball"][:, :, P.NORMAL] * (ref["ball"][:, :, P.GAP] + BC.ball_radius())[..., None]
        assert np.abs(centre - ball[:, None, 0:3].astype(np.float64))[outside].max() < 1e-12
        assert np.abs(np.linalg.norm(ref["ball"][:, :, P.NORMAL], axis=2) - 1).max() < 1e-12


def test_pair_distance_is_bounded_by_a_dense_sampling(generated, contact):
    """201 x 201 points on the two axes: no sampled distance is below the reference's, and the sampled minimum is within the reach of the
    grid (half a step along each axis) of it"""
    K = 201
    u = np.linspace(0.0, 1.0, K)
    for asset, (root, dof) in (("default", generated[0:2]), ("box_cleats", contact["box_cleats"][0:2])):
        T = P.tables(asset)
        n = 40
        E, r = P.link_frames(T, root[:n, 3:7], dof[:n, :, 0])
        c0, c1 = P.capsule_axes(T, E, r, np.float64)
        ia, ib = T["pairs"][:, 0], T["pairs"][:, 1]
        ca, cb, dd = P.segment_closest(c0[:, ia], c1[:, ia], c0[:, ib], c1[:, ib])
        A = c0[:, ia, None, :] + u[None, None, :, None] * (c1[:, ia] - c0[:, ia])[:, :, None, :]
        B = c0[:, ib, None, :] + u[None, None, :, None] * (c1[:, ib] - c0[:, ib])[:, :, None, :]
        sampled = np.stack([np.sqrt(((A[e, :, :, None, :] - B[e, :, None, :, :]) ** 2).sum(-1).min(axis=(1, 2))) for e in range(n)])
        reach = 0.5 / (K - 1) * (np.linalg.norm(c1[:, ia] - c0[:, ia], axis=2) + np.linalg.norm(c1[:, ib] - c0[:, ib], axis=2))
        ref = np.sqrt(dd)
        assert (sampled >= ref - 1e-12).all(), float((ref - sampled).max())
        assert (sampled <= ref + reach).all(), float((sampled - ref - reach).max())
        # the closest points lie on their segments and are that far apart
        assert np.abs(np.linalg.norm(ca - cb, axis=2) - ref).max() < 1e-12


def test_pair_rows_follow_the_definition(contact):
    root, dof, ball, _ = contact["default"]
    T = P.tables("default")
    ref = P.proximity_ref("default", root, dof, ball[:, 0:3])["pairs"]
    E, r = P.link_frames(T, root[:, 3:7], dof[:, :, 0])
    c0, c1 = P.capsule_axes(T, E, r, np.float64)
    ia, ib = T["pairs"][:, 0], T["pairs"][:, 1]
    ca, cb, dd = P.segment_closest(c0[:, ia], c1[:, ia], c0[:, ib], c1[:, ib])
    rs = T["cap_r"][ia] + T["cap_r"][ib]
    assert np.abs(ref[:, :, P.GAP] - (np.sqrt(dd) - rs)).max() < 1e-15
    assert np.abs(np.linalg.norm(ref[:, :, P.NORMAL], axis=2) - 1).max() < 1e-12
    depth = -ref[:, :, P.GAP]
    x = root[:, None, 0:3].astype(np.float64) + cb + ref[:, :, P.NORMAL] * (T["cap_r"][ib] - 0.5 * depth)[..., None]
    assert np.abs(ref[:, :, P.POINT] - x).max() < 1e-12
    assert (ref[:, :, 7] == 0).all()
    # axes that meet: no direction
    p = np.zeros((1, 3)); q = np.array([[1.0, 0, 0]])
    rows = P.pair_rows(dict(T, pairs=np.array([[0, 1]])), np.stack([p, np.array([[0.5, -1.0, 0]])], 1), np.stack([q, np.array([[0.5, 1.0, 0]])], 1),
                       np.zeros((1, 3)), np.float64)
    assert rows[0, 0, P.GAP] == -(T["cap_r"][0] + T["cap_r"][1]) and (rows[0, 0, P.NORMAL] == 0).all() and np.allclose(rows[0, 0, P.POINT], [0.5, 0, 0])


@pytest.mark.parametrize("asset", P.ASSETS)
def test_ground_rows_are_the_rigid_body_pose_applied_to_the_offsets(asset, generated):
    from tests.limb_ik_numpy import quat_to_mat
    root, dof, ball = generated
    root = root.astype(np.float64)
    root[:, 3:7] /= np.linalg.norm(root[:, 3:7], axis=1, keepdims=True)   # (body rows carry unit quaternions; the reference takes the root's as given)
    ref = P.proximity_ref(asset, root, dof, ball[:, 0:3])["ground"]
    rb = _rigid_body_rows(asset, root, dof)
    T = P.tables(asset)
    m = P.MODEL["cleats"] if "cleats" in asset else P.MODEL
    pts = (P.MODEL["cleats"] if "cleats" in asset else P.MODEL)["ground_points"]
    for i in range(P.NPT):
        # the point's own body row (a cleat's for the cleats asset) or its link's: both carry the link's rotation
        b = m["links"][T["pt_link"][i]]["body"]
        Rb = quat_to_mat(rb[:, b, 3:7], np.float64)
        x = rb[:, b, 0:3] + np.einsum("nij,j->ni", Rb, T["pt_pos"][i] - np.asarray(m["body_offset"][b]))
        assert np.abs(ref[:, i] - x).max() < 1e-9, (asset, i)
        assert pts[i]["link"] == T["pt_link"][i]
    R = P.MODEL["ball"]["radius"]
    assert np.abs(ref[:, P.NPT] - (ball[:, 0:3].astype(np.float64) - [0, 0, R])).max() < 1e-15
    # the asset's own tables: cleats move the foot points, the box asset the upper-body points, box + cleats the right ankle
    base = P.proximity_ref("default", root, dof, ball[:, 0:3])["ground"]
    moved = np.abs(ref - base).max(axis=(0, 2)) > 1e-6
    if asset == "default":
        assert not moved.any()
    if "cleats" in asset:
        assert moved[0:8].all()
    if asset == "box":
        assert moved[8:22].any() and not moved[0:8].any()


def test_abi_name_tables_match_the_model():
    m = P.MODEL
    names = m["body_names"]
    link_name = [L["name"] for L in m["links"]]
    seen = {}
    for i, p in enumerate(m["ground_points"]):
        k = seen.get(p["link"], 0)
        seen[p["link"]] = k + 1
        assert abi.PROX_GROUND_NAMES[i] == "%s%s_%d" % (p["kind"], link_name[p["link"]], k)
    assert len(abi.PROX_GROUND_NAMES) == P.NPT == abi.PROX_BALL_ROW == abi.PROX_GROUND_ROWS - 1
    assert abi.PROX_BOX_BODIES == tuple(names[m["links"][b["link"]]["body"]] for b in m["boxes"]) and len(abi.PROX_BOX_BODIES) == abi.PROX_BOXES
    caps = [names[m["links"][c["link"]]["body"]] for c in m["capsules"]]
    assert abi.PROX_PAIR_BODIES == tuple((caps[a], caps[b]) for a, b in m["capsule_pairs"]) and len(abi.PROX_PAIR_BODIES) == abi.PROX_PAIRS
    assert abi.PROX_PAIRS_CAPSULES == tuple(tuple(p) for p in m["capsule_pairs"])
    assert all(a.startswith("/left") and b.startswith("/right") for a, b in abi.PROX_PAIR_BODIES)
    # the cleats asset's bodies of the same names exist
    assert set(abi.PROX_BOX_BODIES) <= set(m["cleats"]["body_names"])
    assert (abi.PROX_WORDS, abi.PROX_GAP, abi.PROX_NORMAL, abi.PROX_POINT) == (8, 0, 1, 4)


@pytest.mark.parametrize("asset", P.ASSETS)
def test_coverage_of_the_gpu_state_sets(asset, generated, contact):
    root, dof, ball, plan = contact[asset]
    ref = P.proximity_ref(asset, root, dof, ball[:, 0:3])
    cond = P.conditioning(asset, root, dof, ball[:, 0:3])
    gap = ref["pairs"][:, :, P.GAP]
    assert ((gap < -1e-3).sum(axis=0) >= 3).all() and ((gap > 1e-3).sum(axis=0) >= 3).all(), ((gap < 0).sum(axis=0), (gap > 0).sum(axis=0))
    # the aimed pair of every env has the aimed sign
    aimed = gap[np.arange(N), plan["pair"]]
    assert ((aimed < 0) == plan["overlap"]).all()
    # every box: through a face (1 coordinate clamped), an edge (2), a corner (3), and with the centre inside (0), on well-conditioned rows
    for b in range(P.NBOX):
        for mode in range(4):
            rows = (cond["ball_mode"][:, b] == mode) & cond["ball_ok"][:, b]
            assert rows.sum() >= 3, (b, mode, int(rows.sum()))
    e = np.arange(N)
    aimed_mode = cond["ball_mode"][e, plan["box"]]
    assert (aimed_mode == np.where(plan["mode"] == 3, 0, plan["mode"] + 1)).all()
    assert cond["ball_ok"][e, plan["box"]].all()
    bg = ref["ball"][e, plan["box"], P.GAP]
    assert (bg < 0).sum() > 50 and (bg > 0).sum() > 20
    # every ground point above and below the plane
    h = cond["height"]
    assert ((h > 1e-3).sum(axis=0) >= 3).all() and ((h < -1e-3).sum(axis=0) >= 3).all()
    # the caps on what the comparison of normals and points leaves out, on both sets
    assert (~cond["pair_ok"]).mean(axis=0).max() <= PAIR_CAP and (~cond["ball_ok"]).mean(axis=0).max() <= BALL_CAP
    g = P.conditioning(asset, generated[0], generated[1], generated[2][:, 0:3])
    assert (~g["pair_ok"]).mean(axis=0).max() <= PAIR_CAP and (~g["ball_ok"]).mean(axis=0).max() <= BALL_CAP
    if asset == "default":
        assert abs((~g["pair_ok"]).mean(axis=0).max() - 0.187) < 0.002   # pair 0: the joints-at-zero seam states
        gen = P.proximity_ref(asset, generated[0], generated[1], generated[2][:, 0:3])
        assert (gen["pairs"][:, 27, P.GAP] > 0).all() and gen["ball"][:, :, P.GAP].min() > 4.0   # why the contact set exists


def test_yardstick_and_mutations(contact):
    root, dof, ball, _ = contact["default"]
    ref = P.proximity_ref("default", root, dof, ball[:, 0:3])
    cond = P.conditioning("default", root, dof, ball[:, 0:3])
    yard = P.yardstick_error(ref, "default", root, dof, ball[:, 0:3], cond)
    assert set(yard) == set(P.BLOCKS) == set(P.block_slices())
    assert 0 < yard["pair_gap"] < 1e-6 and 0 < yard["ball_gap"] < 1e-6 and 0 < yard["ground_z"] < 1e-6
    assert all(v == 0.0 for v in P.block_errors(ref, ref, cond).values())
    for mutate, block in (("capsule_radius", "pair_gap"), ("box_half_extent", "ball_gap"), ("ground_point", "ground_z"), ("normal_reversed", "pair_normal")):
        err = P.block_errors(P.proximity_ref("default", root, dof, ball[:, 0:3], mutate=mutate), ref, cond)
        assert err[block] > 1e-4 and all(v == 0.0 for k, v in err.items() if k.split("_")[0] != block.split("_")[0]), (mutate, err)
