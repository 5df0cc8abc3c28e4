"""GPU: bez_sim_proximity (include/bez_sim.h "Proximity": the ground points, the ball against the eleven boxes, the 28 leg-to-leg capsule
pairs) against the fp64 reference of tests/proximity_numpy.py, against the step's own choice of the deepest box, and its contract to the
bit.

Sizes: 1, 15, 16, 17 (the kernel's 16-env tile), 33, 65, 300 (many tiles, ragged last tile).  Assets default / cleats / box and box +
cleats (the asset whose right ankle's joint origin moves) in the kick and walk layouts.  State sets: "generated"
(tests.state_sets.generate_states: roots up to 100 m out, every attitude seam, joints at their limits; the ball far away) and
"contact" (proximity_numpy.contact_states: every pair overlapping and apart, every box through a face, an edge, a corner and with the
centre inside, every ground point above and below the plane).  No outlier budget anywhere.

  known answer   per block (ground xy, ground z, ball gap / normal / point, pair gap / normal / point): 3x the worst absolute error of
                 proximity_ref evaluated in np.float32 against fp64 on the same inputs + 2 fp32 ulps of the block's largest |reference|.
                 Gaps and ground rows on every env; normals and points where they are well conditioned (proximity_numpy.conditioning);
                 the left-out share is capped at 25 % of any pair and 5 % of any box.

Measured on MI355X: see DESIGN.md 4.3l and profiles/proximity_errors.txt."""
import numpy as np
import pytest
import torch

from bez_isaacgym_amd import abi
from tests import ball_contact_ref as BC
from tests import proximity_numpy as P
from tests.gpu_util import ASSETS, _bits, _host, _sim, _write_states
from tests.sim_cfg import make_cfg
from tests.state_sets import ball_states, generate_states, ulp32

pytestmark = pytest.mark.gpu

TILE = 16
SIZES = (1, TILE - 1, TILE, TILE + 1, 33, 65, 300)
NMAX = max(SIZES)
ASSETS4 = dict(ASSETS, box_cleats=dict(cleats=True, box=True))
SETS = ("generated", "contact")
PAIR_CAP, BALL_CAP = 0.25, 0.05
PARKED = np.array([1000.0, 0.0, np.float32(P.MODEL["ball"]["radius"])], np.float32)   # where a task without a ball keeps it
_CACHE = {}


def _states(name, asset):
    """fp32 (root (NMAX, 13), dof (NMAX, 18, 2), ball (NMAX, 13)); computed once and left unchanged"""
    key = ("states", name, asset if name == "contact" else None)
    if key not in _CACHE:
        if name == "generated":
            root, dof, _ = generate_states(NMAX)
            _CACHE[key] = (root, dof, ball_states(NMAX))
        else:
            _CACHE[key] = P.contact_states(NMAX, asset, seed=7)[0:3]
    return _CACHE[key]


def _ball_pos(name, asset, task):
    return _states(name, asset)[2][:, 0:3] if task == "bez_kick" else np.broadcast_to(PARKED, (NMAX, 3)).copy()


def _bars(ref, yard):
    return {name: 3.0 * yard[name] + 2.0 * float(ulp32(np.abs(ref[w][ix]).max())) for name, (w, ix) in P.block_slices().items()}


def _ref(name, asset, task="bez_kick"):
    """(reference in fp64 for NMAX envs, conditioning, {block: bar}); computed once per key and left unchanged"""
    key = ("ref", name, asset, task)
    if key not in _CACHE:
        root, dof, _ = _states(name, asset)
        bp = _ball_pos(name, asset, task)
        ref = P.proximity_ref(asset, root, dof, bp)
        cond = P.conditioning(asset, root, dof, bp)
        assert (~cond["pair_ok"]).mean(axis=0).max() <= PAIR_CAP and (~cond["ball_ok"]).mean(axis=0).max() <= BALL_CAP
        _CACHE[key] = (ref, cond, _bars(ref, P.yardstick_error(ref, asset, root, dof, bp, cond)))
    return _CACHE[key]


def _prepared(cfg, n, name, asset, root=None, dof=None, ball=None):
    st = _states(name, asset)
    sim = _sim(cfg)
    _write_states(sim, st[0][:n] if root is None else root, st[1][:n] if dof is None else dof, st[2][:n] if ball is None else ball)
    return sim


def _call(sim, **kw):
    g, b, p = sim.proximity(**kw)
    return {k: _host(v) for k, v in (("ground", g), ("ball", b), ("pairs", p)) if v is not None}


def _ratios(got, ref, cond, bars, n):
    return {k: v / bars[k] for k, v in P.block_errors(got, ref, cond, n).items()}


def _env(sim, n):
    """a VecTask around `sim`: the helpers need the sim and the env count only, no task is set up"""
    from bez_isaacgym_amd.tasks.base.vec_task import VecTask

    class Env(VecTask):
        def pre_physics_step(self, actions):
            pass

        def post_physics_step(self):
            pass
    env = Env.__new__(Env)
    env.sim, env.num_environments = sim, n
    return env


def _same(a, b):
    return all((_bits(a[k]) == _bits(b[k])).all() for k in a)


@pytest.mark.parametrize("task", ["bez_kick", "bez_walk"])
@pytest.mark.parametrize("asset", list(ASSETS4))
def test_known_answer(asset, task):
    """both state sets at every size: every block of every env against proximity_ref in fp64 on the fp32 state; the walk layout has the
    ball parked at (1000, 0, R) and reports its rows like any other"""
    report = {}
    for name in SETS:
        ref, cond, bars = _ref(name, asset, task)
        for n in SIZES:
            sim = _prepared(make_cfg(n, task=task, seed=5, **ASSETS4[asset]), n, name, asset)
            got = _call(sim)
            sim.close()
            assert got["ground"].shape == (n, 23, 3) and got["ball"].shape == (n, 11, 8) and got["pairs"].shape == (n, 28, 8)
            assert all(v.dtype == np.float32 for v in got.values())
            assert (_bits(got["ball"][:, :, 7]) == 0).all() and (_bits(got["pairs"][:, :, 7]) == 0).all()
            for b, v in _ratios(got, ref, cond, bars, n).items():
                report[name, b] = max(report.get((name, b), 0.0), v)
        print("PROX_KNOWN_ANSWER %-10s %-8s %-9s worst error / bar: %s" % (asset, task, name, " ".join("%s %.3f" % (b, report[name, b]) for b in P.BLOCKS)))
        print("PROX_KNOWN_ANSWER %-10s %-8s %-9s bars: %s; left out: pairs %.3f, ball rows %.3f" %
              (asset, task, name, {k: float("%.3g" % v) for k, v in bars.items()}, (~cond["pair_ok"]).mean(axis=0).max(), (~cond["ball_ok"]).mean(axis=0).max()))
    assert max(report.values()) <= 1.0, {k: v for k, v in report.items() if v > 1.0}


@pytest.mark.parametrize("asset", list(ASSETS))
def test_the_steps_choice(asset):
    """VecTask.ball_gap()'s box is the deepest box of tests/ball_contact_ref.depths (the independent sphere-box test the step kernels are
    held to) wherever that choice is not a knife edge (kept: KEPT_MARGIN); and the sign of every ground z is the sign of the fp64 height
    wherever the height exceeds the block's bar"""
    n = NMAX
    fs = BC.free_space_states(n, asset, 4)
    sets = {"free_space": (fs["root_states"][:, 0], fs["dof_state"], fs["root_states"][:, 1]), "contact": _states("contact", asset)}
    for name, (root, dof, ball) in sets.items():
        sim = _sim(make_cfg(n, seed=5, **ASSETS[asset]))
        _write_states(sim, root, dof, ball)
        env = _env(sim, n)
        gap, idx = (_host(t) for t in env.ball_gap())
        rb = _host(sim.refresh(abi.TENSOR_RIGID_BODY_STATE)).reshape(n, -1, 13)
        ground = _call(sim, want=("ground",))["ground"]
        sim.close()
        d = BC.depths(rb, ball[:, 0:3], asset)
        kept, win = BC.kept(d), BC.winner(d)
        hit = kept & (win >= 0) & (d.max(axis=1) > BC.KEPT_MARGIN)
        assert hit.sum() >= n // 3, (name, int(hit.sum()))
        assert (idx[hit] == win[hit]).all(), (name, np.flatnonzero(hit & (idx != win))[:5])
        assert np.abs(-gap[hit] - d.max(axis=1)[hit]).max() < 2e-5   # (the depths come from fp32 body rows up to 100 m out)
        clear = kept & (d.max(axis=1) < -BC.KEPT_MARGIN)
        assert (gap[clear] > 0).all()
        ref, cond, bars = (P.proximity_ref(asset, root, dof, ball[:, 0:3]), P.conditioning(asset, root, dof, ball[:, 0:3]), None)
        yard = P.yardstick_error(ref, asset, root, dof, ball[:, 0:3], cond)
        bar = _bars(ref, yard)["ground_z"]
        h = cond["height"]
        sure = np.abs(h) > bar
        assert sure.mean() > 0.99 and (np.sign(ground[:, :22, 2])[sure] == np.sign(h)[sure]).all()
        print("PROX_STEP_CHOICE %-8s %-10s deepest box agrees on %d envs; ground signs agree on %d of %d points (bar %.3g m)" % (asset, name, hit.sum(), sure.sum(), sure.size, bar))


def test_to_the_bit():
    """pad words; the z words under a change of root_pos.x / root_pos.y; N, the place in the tile and the outputs' alignment; an output
    that was not asked for; the state and every tensor after the call; a NaN in one env's q"""
    n, asset = 65, "cleats"
    root, dof, ball = (a[:n] for a in _states("contact", asset))
    cfg = lambda k: make_cfg(k, seed=5, **ASSETS4[asset])
    sim = _prepared(cfg(n), n, "contact", asset)
    snap = lambda: [_host(sim.refresh(w)) for w in (abi.TENSOR_ROOT_STATE, abi.TENSOR_DOF_STATE, abi.TENSOR_RIGID_BODY_STATE, abi.TENSOR_NET_CONTACT_FORCE)] \
        + [_host(sim.tensor(w)) for w in (abi.TENSOR_OBS, abi.TENSOR_REW, abi.TENSOR_RESET, abi.TENSOR_PROGRESS)] + [_host(sim.inverse_dynamics(None, abi.ID_ALL))]
    before = snap()
    a = _call(sim)
    for x, y in zip(before, snap()):
        assert (x.view(np.uint8) == y.view(np.uint8)).all()
    assert (_bits(a["ball"][:, :, 7]) == 0).all() and (_bits(a["pairs"][:, :, 7]) == 0).all()
    # outputs 4 bytes off a 16-byte boundary
    off4 = lambda shape: torch.zeros(torch.Size(shape).numel() + 1, device="cuda:0")[1:].view(shape)
    b = _call(sim, ground=off4((n, 23, 3)), ball=off4((n, 11, 8)), pairs=off4((n, 28, 8)))
    assert _same(a, b)
    # one output at a time: the same bits, and what was not asked for is untouched (the sim's own buffers hold a marker)
    for w in ("ground", "ball", "pairs"):
        for k in ("ground", "ball", "pairs"):
            sim._buffers["proximity_" + k].fill_(-7.0)
        one = _call(sim, want=(w,))
        assert list(one) == [w] and (_bits(one[w]) == _bits(a[w])).all()
        for k in ("ground", "ball", "pairs"):
            if k != w:
                assert (_host(sim._buffers["proximity_" + k]) == -7.0).all()
    # root_pos.x / root_pos.y: the z words and everything relative to the root keep their bits
    moved = root.copy()
    moved[:, 0:2] = moved[::-1, 0:2] * 0.37 + 3.0
    _write_states(sim, moved, dof, ball)
    c = _call(sim)
    assert (_bits(c["ground"][:, :22, 2]) == _bits(a["ground"][:, :22, 2])).all()
    assert (_bits(c["pairs"][:, :, 0:4]) == _bits(a["pairs"][:, :, 0:4])).all() and (_bits(c["pairs"][:, :, 6]) == _bits(a["pairs"][:, :, 6])).all()
    assert np.abs(c["ground"][:, :22, 0:2] - a["ground"][:, :22, 0:2]).max() > 1.0
    # a NaN in one env's q: that env's rows of the right leg are non-finite, its pad words +0.0f, every other env keeps its bits
    bad = dof.copy()
    bad[40, 12, 0] = np.nan
    _write_states(sim, root, bad, ball)
    d = _call(sim)
    others = np.arange(n) != 40
    assert all((_bits(d[k][others]) == _bits(a[k][others])).all() for k in a)
    assert not np.isfinite(d["pairs"][40, :, 0]).any() and not np.isfinite(d["ball"][40, 5:10, 0:7]).any() and not np.isfinite(d["ground"][40, 4:8]).any()
    assert (_bits(d["ball"][40, :, 7]) == 0).all() and (_bits(d["pairs"][40, :, 7]) == 0).all()
    assert (_bits(d["ball"][40, 0:5]) == _bits(a["ball"][40, 0:5])).all() and (_bits(d["ground"][40, 0:4]) == _bits(a["ground"][40, 0:4])).all()
    sim.close()
    # N and the place in the tile: 17 envs alone, and the same envs 5 places further on
    sim = _prepared(cfg(17), 17, "contact", asset)
    s = _call(sim)
    sim.close()
    assert all((_bits(s[k]) == _bits(a[k][:17])).all() for k in a)
    roll = lambda x: np.roll(x, 5, axis=0)
    sim = _prepared(cfg(n), n, "contact", asset, roll(root), roll(dof), roll(ball))
    r = _call(sim)
    sim.close()
    assert all((_bits(r[k]) == _bits(roll(a[k]))).all() for k in a)


def test_contract():
    """the argument errors; BEZ_FLAG_NO_SELF_COLLISION changes no output bit; the call captures into a graph on one stream and the replay
    reproduces the bits"""
    from bez_isaacgym_amd.sim import BezSimError
    import ctypes as C
    n, asset = 33, "default"
    sim = _prepared(make_cfg(n, seed=5), n, "contact", asset)
    a = _call(sim)
    g, b, p = (torch.zeros(n, r, w, device="cuda:0") for r, w in ((23, 3), (11, 8), (28, 8)))
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    call = lambda h, x, y, z: sim.lib.bez_sim_proximity(h, ptr(x), ptr(y), ptr(z), None)
    assert call(sim.h, g, b, p) == 0 and call(sim.h, g, None, None) == 0 and call(sim.h, None, b, None) == 0 and call(sim.h, None, None, p) == 0
    torch.cuda.synchronize()
    assert (_bits(_host(g)) == _bits(a["ground"])).all() and (_bits(_host(b)) == _bits(a["ball"])).all() and (_bits(_host(p)) == _bits(a["pairs"])).all()
    assert call(sim.h, None, None, None) == -1
    assert b"bez_sim_proximity" in sim.lib.bez_sim_last_error(sim.h)
    assert call(None, g, b, p) == -1
    assert b"bez_sim_proximity" in sim.lib.bez_sim_last_error(None)
    for kw in (dict(ground=g[:, :22]), dict(ball=b.view(n, 8, 11)), dict(pairs=p[:-1]), dict(want=("ground", "legs")), dict(want=()),
               dict(ground=a["ground"])):
        with pytest.raises(BezSimError):
            sim.proximity(**kw)
    # one stream, one captured launch; the replay sees the state as it stands then
    root, dof, ball = (x[:n] for x in _states("generated", asset))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        sim.proximity(g, b, p)
    _write_states(sim, root, dof, ball)
    graph.replay()
    got = dict(ground=_host(g), ball=_host(b), pairs=_host(p))
    direct = _call(sim)
    assert _same(got, direct) and not _same(got, a)
    sim.close()
    cfg = make_cfg(n, seed=5)
    cfg.flags |= abi.FLAG_NO_SELF_COLLISION
    sim = _prepared(cfg, n, "contact", asset)
    assert _same(_call(sim), a)
    sim.close()


SENSITIVITY = (("capsule_radius", "pair_gap"), ("box_half_extent", "ball_gap"), ("ground_point", "ground_z"), ("normal_reversed", "pair_normal"))


@pytest.mark.parametrize("mutate,block", SENSITIVITY, ids=[s[0] for s in SENSITIVITY])
def test_sensitivity(mutate, block):
    """one capsule radius 1 % off, one box half extent 1 mm off, one ground point moved 0.5 mm, one pair's normal reversed -- each in the
    reference alone -- puts the GPU's result outside the bar of its block: a kernel with that slip would not pass the known-answer test"""
    n, asset = 65, "default"
    ref, cond, bars = _ref("contact", asset)
    root, dof, ball = _states("contact", asset)
    wrong = P.proximity_ref(asset, root, dof, ball[:, 0:3], mutate=mutate)
    sim = _prepared(make_cfg(n, seed=5), n, "contact", asset)
    got = _call(sim)
    sim.close()
    right, off = _ratios(got, ref, cond, bars, n), _ratios(got, wrong, cond, bars, n)
    print("PROX_SENSITIVITY %-16s worst error / bar against the reference %.3f, against the reference with the slip: %s %.1f" % (mutate, max(right.values()), block, off[block]))
    assert max(right.values()) <= 1.0 and off[block] > 1.0, (right, off)


def test_vec_task_helpers():
    """foot_clearance, self_collision_gap and ball_gap against the raw tensors"""
    n, asset = 33, "default"
    sim = _prepared(make_cfg(n, seed=5), n, "contact", asset)
    env = _env(sim, n)
    raw = {k: _host(v) for k, v in zip(("ground", "ball", "pairs"), env.proximity())}
    fc = _host(env.foot_clearance())
    sg = _host(env.self_collision_gap())
    bg, bi = (_host(t) for t in env.ball_gap())
    sim.close()
    assert fc.shape == (n, 2) and (fc[:, 0] == raw["ground"][:, 0:4, 2].min(axis=1)).all() and (fc[:, 1] == raw["ground"][:, 4:8, 2].min(axis=1)).all()
    assert sg.shape == (n,) and (sg == raw["pairs"][:, :, 0].min(axis=1)).all() and (sg < 0).any() and (sg > 0).any()
    assert bg.shape == bi.shape == (n,) and (bg == raw["ball"][:, :, 0].min(axis=1)).all() and (bi == raw["ball"][:, :, 0].argmin(axis=1)).all()
    assert len(abi.PROX_GROUND_NAMES) == 22 and len(abi.PROX_BOX_BODIES) == 11 and len(abi.PROX_PAIR_BODIES) == 28
