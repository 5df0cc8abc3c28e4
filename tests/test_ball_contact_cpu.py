"""The ball-contact state generators and the numpy sphere-box reference of tests/ball_contact_ref.py, held against the fp64 oracle alone
(no GPU): the generated states reach every box and every hand-over between the kernels' box owners, and the numpy test's deepest box
is the one body the oracle loads.  tests/test_gpu_ball_contact.py runs the same states through the step kernels."""
import numpy as np
import pytest

from bez_isaacgym_amd import abi
from oracle.bez_oracle import Oracle
from tests import ball_contact_ref as B
from tests import step_terms as S

N = 1056   # 96 envs aim at each box
SEED = 4


@pytest.fixture(scope="module", params=list(S.ASSETS))
def free_space(request):
    """free-space states in a one-substep oracle without leg<->leg contact, their depths, and the contact rows of one step"""
    asset = request.param
    st = B.free_space_states(N, asset, SEED)
    o = Oracle(S.step_cfg(N, asset, gravity=False, substeps=1, flags=abi.FLAG_NO_SELF_COLLISION))
    S.inject(o, st)
    rb = o.rigid_body_states.reshape(N, -1, 13)
    d = B.depths(rb, st["root_states"][:, 1, 0:3], asset)
    o.pre_physics(S.actions(N, 2)); o.simulate()
    return asset, st, rb, d, o.contact_forces.reshape(N, -1, 3).astype(np.float64)


def test_generator_kinematics_match_the_rigid_body_rows(free_space):
    """the generator's forward kinematics of the model JSON put every link where the oracle's rigid-body rows have it (fp32 rows: 6e-8),
    and the ball sits 0.5 - 10 mm deep in the box it was aimed at"""
    asset, st, rb, d, _ = free_space
    rs, ds = st["root_states"], st["dof_state"]
    _, r = B.link_frames(asset, rs[:, 0, 0:3], rs[:, 0, 3:7], ds[:, :, 0])
    for i, L in enumerate(B.asset_links(asset)):
        np.testing.assert_allclose(r[:, i], rb[:, L["body"], 0:3], atol=5e-7, err_msg=L["name"])
    aimed = d[np.arange(N), st["aim"]]
    assert 0.5e-3 - 1e-6 <= aimed.min() and aimed.max() <= 10e-3 + 1e-6, (aimed.min(), aimed.max())


def test_generator_conditions(free_space):
    """what the GPU tests rely on (measured: dropped 2.6 - 2.7 %, least-hit box 15 kept envs, another owner's candidate positive in
    66 % (cleats) - 79 % of the envs, centre inside a box 14 - 15 %)"""
    asset, st, rb, d, _ = free_space
    k, w, g = B.kept(d), B.winner(d), B.owner_groups(asset)
    assert (d.max(1) > 0).all()
    assert 1.0 - k.mean() <= 0.05, 1.0 - k.mean()
    wins = np.bincount(w[k], minlength=B.NBOX)
    assert wins.min() >= 10, wins
    other_owner = ((d > 0) & (g[None, :] != g[w][:, None])).any(1)
    assert other_owner.mean() >= 0.40, other_owner.mean()
    assert B.centre_inside(d).mean() >= 0.05, B.centre_inside(d).mean()


def test_numpy_winner_is_the_loaded_row(free_space):
    """one substep, no leg<->leg contact, no ground: in every kept env the only loaded robot row is the body of the numpy winner, or none
    (the oracle rejects a contact whose bodies separate fast enough: measured 6 % of the envs), and the ball row is its exact negative"""
    asset, st, rb, d, cf = free_space
    k = B.kept(d)
    nb = B.ball_row(asset)
    loaded = B.loaded_rows(cf, asset)
    count = loaded.sum(1)
    want = B.winner_body(d, asset)
    assert (count[k] <= 1).all()
    hit = k & (count == 1)
    np.testing.assert_array_equal(loaded.argmax(1)[hit], want[hit])
    np.testing.assert_array_equal(cf[k, nb], -cf[k, :nb].sum(1))
    rejected = (count[k] == 0).mean()
    assert 0.02 <= rejected <= 0.15, rejected


@pytest.mark.parametrize("asset", list(S.ASSETS))
def test_kick_stance_reaches_the_lower_leg_boxes(asset):
    """standing robot, ball on the ground next to a foot: the calf, ankle and foot boxes of both legs each win in >= 3 kept envs (measured:
    calf 289 / 273, ankle 223 / 213, foot 10 / 4 of 1056), and the ball touches the ground"""
    st = B.kick_stance_states(N, asset, 3)
    o = Oracle(S.step_cfg(N, asset))
    S.inject(o, st)
    d = B.depths(o.rigid_body_states.reshape(N, -1, 13), st["root_states"][:, 1, 0:3], asset)
    k, w = B.kept(d), B.winner(d)
    wins = np.bincount(w[k & (w >= 0)], minlength=B.NBOX)
    assert (wins[[2, 3, 4, 7, 8, 9]] >= 3).all(), wins
    assert 1.0 - k.mean() <= 0.05
    z = st["root_states"][:, 1, 2]
    assert (z <= B.ball_radius()).all() and (z >= B.ball_radius() - 2e-3 - 1e-6).all()


def test_park_ball_touches_only_the_unlisted_envs():
    st = B.free_space_states(24, "default", 1)
    parked = B.park_ball(st, [0, 5, 23])
    np.testing.assert_array_equal(parked["root_states"][[0, 5, 23]], st["root_states"][[0, 5, 23]])
    np.testing.assert_array_equal(parked["root_states"][:, 0], st["root_states"][:, 0])
    rest = np.setdiff1d(np.arange(24), [0, 5, 23])
    np.testing.assert_array_equal(parked["root_states"][rest, 1, 0:3], np.tile(np.float32(B.PARKED), (len(rest), 1)))
    assert not parked["root_states"][rest, 1, 7:].any()
