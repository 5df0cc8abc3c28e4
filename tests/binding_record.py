"""Support: what the Python binding (bez_isaacgym_amd/sim.py, the parsers of abi.py) does with its arguments, recorded without a device.
A BezSim made with __new__ over a fake library runs a fixed table of calls; record() returns, JSON-able, what reached the library
and what came back, or how the call was refused.  tests/golden/binding_calls.json is this record of the commit before the binding
was folded (tests/test_binding_cpu.py compares); only public methods are called, so the module runs on any tree:

    PYTHONPATH=<tree> python tests/binding_record.py > binding_calls.json       # the record of <tree>
    PYTHONPATH=<tree> python tests/binding_record.py --time                    # host seconds per query call on the fake library
"""
import ctypes as C
import itertools
import json
import math
import sys
import time

import numpy as np
import torch

N, NB_BALL, NB_NO_BALL = 3, 22, 21


class FakeLib:
    """every bez_sim_* entry point: records (name, args) and returns `rc`"""

    def __init__(self, rc=0):
        self.calls, self.rc = [], rc

    def bez_sim_last_error(self, h):
        return b"the fake library was told to fail"

    def __getattr__(self, name):
        if not name.startswith("bez_sim_"):
            raise AttributeError(name)

        def entry(*args):
            self.calls.append((name, args))
            return self.rc
        self.__dict__[name] = entry
        return entry


def bare_sim(ball=True, rc=0):
    """a BezSim without a device: its argument checks run before anything reaches the library"""
    from bez_isaacgym_amd.sim import BezSim
    s = BezSim.__new__(BezSim)
    s.lib, s.h, s.num_envs, s.num_bodies, s.has_ball = FakeLib(rc), None, N, NB_BALL if ball else NB_NO_BALL, ball
    s.device, s._views, s._stream = torch.device("cpu"), {}, lambda: None
    return s


# ---- the call table


def z(*shape, dtype=torch.float32):
    return torch.zeros(shape, dtype=dtype)


def wrong(shape, every=True):
    """the ways a tensor argument of `shape` is refused: all of them, or (every=False) one of each stage -- shape, pointer, type"""
    swapped = shape[:-2] + (shape[-1], shape[-2])
    few = (z(*shape[:-1], shape[-1] + 1), z(*shape, dtype=torch.float64), np.zeros(shape, np.float32))
    return few + (z(math.prod(shape)), z(shape[0] + 1, *shape[1:]), z(*shape, dtype=torch.int32), z(*swapped).transpose(-1, -2),
                  torch.zeros(shape, device="meta")) if every else few


def mixed_case(name):
    return (name, name.upper(), " " + name.capitalize() + " ")


def subsets(names):
    return [c for k in range(len(names) + 1) for c in itertools.combinations(names, k)]


W_ALL = [[1.0, 1.0]] * 5
OFFSETS = [[0.01 * c, -0.02, 0.03 * c] for c in range(5)]
SPACES = (0, 1) + mixed_case("env") + mixed_case("local") + mixed_case("env_space") + mixed_case("local_space")
BAD_SPACES = ("world", "", 2, -1, 1.0, None, True)
IK_SPACES = (0, 1) + mixed_case("env") + mixed_case("root")
BAD_IK_SPACES = ("local", "", 2, -1, 1.0, None, False)
ATS = mixed_case("com") + mixed_case("origin")
BAD_ATS = ("centre", "", 0, None)
OS_SHAPES = {"jac": (N, 5, 6, 24), "jminv": (N, 5, 6, 24), "w": (N, 30, 30), "lam": (N, 5, 6, 6)}
PROX_SHAPES = {"ground": (N, 23, 3), "ball": (N, 11, 8), "pairs": (N, 28, 8)}


def call_table():
    """[(method, ball, kwargs)]: every sim (one per method and body count) sees its calls in this order"""
    t = []

    def add(method, with_ball=True, **kw):
        t.append((method, with_ball, kw))

    seen = set()

    def add_wrong(method, arg, shape, **kw):
        for bad in wrong(shape, every=method not in seen):   # every way for a method's first tensor argument, one per stage for the others
            add(method, **dict(kw, **{arg: bad}))
        seen.add(method)

    vec = (N, 24)
    # inverse_dynamics(udot, terms, out)
    add("inverse_dynamics"); add("inverse_dynamics")
    for terms in range(8):
        add("inverse_dynamics", terms=terms)
    add("inverse_dynamics", udot=z(*vec)); add("inverse_dynamics", out=z(*vec)); add("inverse_dynamics", udot=z(*vec), terms=1, out=z(*vec))
    add("inverse_dynamics", udot=z(N + 1, 24)[1:])
    add_wrong("inverse_dynamics", "udot", vec); add_wrong("inverse_dynamics", "out", vec)
    add("inverse_dynamics", udot=z(*vec, dtype=torch.float64), out=z(N, 23))     # wrong in two ways: the shapes come first
    add("inverse_dynamics", udot=z(N, 23), out=np.zeros(vec, np.float32))
    add("inverse_dynamics", udot=z(24, N).t(), out=z(*vec, dtype=torch.float16))
    add("inverse_dynamics")
    # forward_dynamics(force, bias, fixed_base, out)
    add("forward_dynamics"); add("forward_dynamics")
    for bias in (2, 4, 6):
        add("forward_dynamics", bias=bias); add("forward_dynamics", force=z(*vec), bias=bias)
    add("forward_dynamics", force=z(*vec), bias=0)
    for fixed in (True, False, 1, 0):
        add("forward_dynamics", fixed_base=fixed); add("forward_dynamics", force=z(*vec), bias=0, fixed_base=fixed, out=z(*vec))
    add("forward_dynamics", out=z(*vec))
    f = z(*vec)
    add("forward_dynamics", force=f, out=f); add("forward_dynamics", force=f, bias=0, fixed_base=True, out=f)
    for bias in (1, 7, 8, -1):
        add("forward_dynamics", bias=bias); add("forward_dynamics", force=z(*vec), bias=bias)
    add("forward_dynamics", bias=0); add("forward_dynamics", bias=0, out=z(*vec))
    add_wrong("forward_dynamics", "force", vec); add_wrong("forward_dynamics", "out", vec)
    add("forward_dynamics", force=z(N, 23), bias=8)                               # the shapes, then the bias, then dtype and layout
    add("forward_dynamics", force=z(*vec, dtype=torch.float64), bias=8)
    add("forward_dynamics", bias=0, out=z(N, 23))
    add("forward_dynamics", force=z(*vec, dtype=torch.float64), out=z(N, 23))
    add("forward_dynamics")
    # operational_space(offsets, fixed_base, jac, jminv, w, lam, want)
    add("operational_space"); add("operational_space")
    for want in subsets(("jac", "jminv", "w", "lambda")):
        add("operational_space", want=want)
        if len(want) == 2:
            add("operational_space", want=list(want))
        if "lambda" not in want:
            add("operational_space", fixed_base=True, want=want)
    for name in ("jac", "jminv", "w", "lambda"):
        add("operational_space", want=name)
    for k in range(5):
        for given in itertools.combinations(OS_SHAPES, k):
            add("operational_space", want=(), **{g: z(*OS_SHAPES[g]) for g in given})
    add("operational_space", jac=z(*OS_SHAPES["jac"]), lam=z(*OS_SHAPES["lam"]), want=("w", "jac"))
    add("operational_space", offsets=OFFSETS); add("operational_space", offsets=torch.tensor(OFFSETS), fixed_base=1, want="w")
    add("operational_space", offsets=np.asarray(OFFSETS), fixed_base=0)
    for offsets in (3, 1.5, "abc", [], OFFSETS[:4], [r[:2] for r in OFFSETS], [[0.0] * 3] * 4 + [[0.0, math.inf, 0.0]],
                    [[0.0] * 3] * 2 + [[math.nan, 0.0, 0.0]] + [[0.0] * 3] * 2, [1, 2, 3, 4, 5]):
        add("operational_space", offsets=offsets)
    for fixed in (None, "yes", 1.0):
        add("operational_space", fixed_base=fixed, want="jac")
    for want in ("lam", "J", ("jac", "W"), ("jac", "lam"), ["bogus"]):
        add("operational_space", want=want)
    add("operational_space", want=()); add("operational_space", want=[]); add("operational_space", want="")
    add("operational_space", fixed_base=True); add("operational_space", fixed_base=True, want="lambda")
    add("operational_space", fixed_base=True, lam=z(*OS_SHAPES["lam"]), want=())
    for arg, shape in OS_SHAPES.items():
        add_wrong("operational_space", arg, shape, want=())
    add("operational_space", offsets=3, want="bogus")                              # the order of the checks
    add("operational_space", want=("lambda", "bogus"), fixed_base=True)
    add("operational_space", want="bogus", jac=z(N, 5, 6, 23))
    add("operational_space", want=(), jac=z(N, 5, 6, 23), w=np.zeros((N, 30, 30), np.float32))
    add("operational_space", want="lambda", fixed_base=True, jac=z(N, 5, 6, 23))
    add("operational_space", want="lambda", fixed_base=True, jac=z(*OS_SHAPES["jac"], dtype=torch.float64))
    add("operational_space", want="w", jac=z(*OS_SHAPES["jac"], dtype=torch.float64), jminv=z(N, 5, 6, 23))
    add("operational_space")
    # centroidal(state, matrix, want_matrix)
    add("centroidal"); add("centroidal")
    add("centroidal", want_matrix=True); add("centroidal", want_matrix=True); add("centroidal", want_matrix=False)
    add("centroidal", state=z(N, 16)); add("centroidal", matrix=z(N, 6, 24)); add("centroidal", state=z(N, 16), matrix=z(N, 6, 24))
    add("centroidal", state=z(N, 16), want_matrix=True); add("centroidal", matrix=z(N, 6, 24), want_matrix=True)
    add_wrong("centroidal", "state", (N, 16)); add_wrong("centroidal", "matrix", (N, 6, 24))
    add("centroidal", state=z(N, 16, dtype=torch.float64), matrix=z(N, 6, 23))
    add("centroidal", state=z(N, 16, dtype=torch.float64), matrix=z(N, 6, 24, dtype=torch.int32), want_matrix=True)
    add("centroidal")
    # body_accelerations(udot, terms, space, out): the robot's bodies, no ball row
    for ball in (True, False):
        add("body_accelerations", ball); add("body_accelerations", ball)
        add("body_accelerations", ball, udot=z(*vec), out=z(N, 21, 6))
        add("body_accelerations", ball, out=z(N, 22, 6))
    for terms in range(8):
        add("body_accelerations", terms=terms)
    for space in SPACES:
        add("body_accelerations", udot=z(*vec), terms=7, space=space, out=z(N, 21, 6))
    for space in BAD_SPACES:
        add("body_accelerations", space=space)
    add_wrong("body_accelerations", "udot", vec); add_wrong("body_accelerations", "out", (N, 21, 6))
    add("body_accelerations", space="world", udot=z(N, 23))
    add("body_accelerations", udot=z(*vec, dtype=torch.float64), out=z(N, 22, 6))
    add("body_accelerations")
    # generalized_forces(forces, torques, positions, space, at, out) and apply_body_forces(forces, torques, positions, space)
    for ball, nb in ((True, NB_BALL), (False, NB_NO_BALL)):
        flat, cube = (N * nb, 3), (N, nb, 3)
        for given in subsets(("forces", "torques", "positions")) if ball else [("forces", "torques", "positions")]:
            for shape in (flat, cube):
                kw = {g: z(*shape) for g in given}
                add("apply_body_forces", ball, **kw)
                add("generalized_forces", ball, **kw)
                add("generalized_forces", ball, at="origin", **kw)
        add("generalized_forces", ball, forces=z(*flat), torques=z(*cube), out=z(*vec))
        add("generalized_forces", ball, forces=z(*cube), positions=z(*flat), space="local", out=z(*vec))
        add("apply_body_forces", ball, forces=z(*flat), torques=z(*cube), positions=z(*flat), space=1)
        other = (N, NB_BALL + NB_NO_BALL - nb, 3)
        add("apply_body_forces", ball, forces=z(*other)); add("generalized_forces", ball, torques=z(*other))
    cube = (N, NB_BALL, 3)
    add("apply_body_forces"); add("apply_body_forces"); add("generalized_forces", forces=z(*cube)); add("generalized_forces", forces=z(*cube))
    for space in SPACES:
        add("apply_body_forces", forces=z(*cube), space=space)
        add("generalized_forces", torques=z(*cube), space=space)
    for space in SPACES[:4]:
        add("generalized_forces", torques=z(*cube), space=space, at="origin")
    for at in ATS:
        add("generalized_forces", forces=z(*cube), at=at); add("generalized_forces", forces=z(*cube), space=1, at=at, out=z(*vec))
        add("generalized_forces", forces=z(*cube), positions=z(*cube), at=at)
    for space in BAD_SPACES:
        add("apply_body_forces", forces=z(*cube), space=space); add("generalized_forces", forces=z(*cube), space=space)
    for at in BAD_ATS:
        add("generalized_forces", forces=z(*cube), at=at)
    for arg in ("forces", "torques", "positions"):
        add_wrong("apply_body_forces", arg, cube); add_wrong("apply_body_forces", arg, (N * NB_BALL, 3))
        add_wrong("generalized_forces", arg, cube, **({} if arg == "forces" else {"forces": z(*cube)}))
    add_wrong("generalized_forces", "out", vec, forces=z(*cube))
    add("generalized_forces", at="centre", space="world")                          # the order of the checks
    add("generalized_forces", space="world"); add("generalized_forces", at="origin", positions=z(*cube))
    add("generalized_forces", forces=z(N, 20, 3), positions=z(*cube), at="origin")
    add("generalized_forces", forces=z(*cube, dtype=torch.float64), torques=z(N, 20, 3))
    add("generalized_forces", forces=z(*cube), positions=z(*cube, dtype=torch.float64), out=z(N, 23))
    add("apply_body_forces", forces=z(*cube, dtype=torch.float64), torques=z(N, 20, 3), space="world")
    add("apply_body_forces", forces=z(*cube, dtype=torch.float64), torques=z(N, 20, 3))
    add("generalized_forces", forces=z(*cube)); add("apply_body_forces", forces=z(*cube))
    # limb_ik(targets, weights, offsets, damping, max_step, iters, space, out, err_out)
    tg = (N, 5, 7)
    add("limb_ik", targets=z(*tg), weights=W_ALL); add("limb_ik", targets=z(*tg), weights=W_ALL)
    add("limb_ik", targets=z(N * 5, 7), weights=W_ALL)
    add("limb_ik", targets=z(*tg), weights=W_ALL, out=z(N, 18)); add("limb_ik", targets=z(*tg), weights=W_ALL, err_out=z(N, 5, 6))
    add("limb_ik", targets=z(N * 5, 7), weights=torch.tensor(W_ALL), offsets=OFFSETS, damping=0.1, max_step=0.2, iters=8, space="root",
        out=z(N, 18), err_out=z(N, 5, 6))
    add("limb_ik", targets=z(*tg), weights=np.asarray([[1.0, 0.0], [0.0, 0.0], [0.5, 2.0], [0.0, 1.0], [3.0, 3.0]]), offsets=np.asarray(OFFSETS),
        max_step=-1.0, iters=np.int64(0))
    for iters in (0, 64, np.int32(3), torch.tensor(5)):
        add("limb_ik", targets=z(*tg), weights=W_ALL, iters=iters)
    for space in IK_SPACES:
        add("limb_ik", targets=z(*tg), weights=W_ALL, space=space)
    for space in BAD_IK_SPACES:
        add("limb_ik", targets=z(*tg), weights=W_ALL, space=space)
    neg, nan = [list(r) for r in W_ALL], [list(r) for r in W_ALL]
    neg[2][1], nan[0][0] = -1.0, math.nan
    for weights in (None, W_ALL[:4], [[1.0] * 3] * 5, [], neg, nan, [[1.0, math.inf]] * 5):
        add("limb_ik", targets=z(*tg), weights=weights)
    for offsets in (3, [], OFFSETS[:4], [r[:2] for r in OFFSETS], [[0.0] * 3] * 4 + [[0.0, math.inf, 0.0]],
                    [[0.0] * 3] * 2 + [[math.nan, 0.0, 0.0]] + [[0.0] * 3] * 2):
        add("limb_ik", targets=z(*tg), weights=W_ALL, offsets=offsets)
    for damping in (0.0, -0.1, math.inf, math.nan):
        add("limb_ik", targets=z(*tg), weights=W_ALL, damping=damping)
    add("limb_ik", targets=z(*tg), weights=W_ALL, max_step=math.nan); add("limb_ik", targets=z(*tg), weights=W_ALL, max_step=math.inf)
    for iters in (-1, 65, 1.5, True, None, "2", np.float64(2.0), np.int64(65)):
        add("limb_ik", targets=z(*tg), weights=W_ALL, iters=iters)
    add_wrong("limb_ik", "targets", tg, weights=W_ALL); add_wrong("limb_ik", "targets", (N * 5, 7), weights=W_ALL)
    add_wrong("limb_ik", "out", (N, 18), targets=z(*tg), weights=W_ALL); add_wrong("limb_ik", "err_out", (N, 5, 6), targets=z(*tg), weights=W_ALL)
    add("limb_ik", targets=z(N, 5, 6), weights=None)                               # the order of the checks
    add("limb_ik", targets=z(N, 5, 6), weights=W_ALL, damping=0.0, iters=-1, space=2)
    add("limb_ik", targets=z(*tg, dtype=torch.float64), weights=W_ALL, out=z(N, 17))
    add("limb_ik", targets=z(*tg), weights=W_ALL, out=z(N, 18, dtype=torch.float64), err_out=z(N, 5, 5))
    add("limb_ik", targets=z(*tg), weights=W_ALL)
    # proximity(ground, ball, pairs, want)
    for ball in (True, False):
        add("proximity", ball); add("proximity", ball)
    for want in subsets(("ground", "ball", "pairs")):
        add("proximity", want=want); add("proximity", want=list(want))
    for name in PROX_SHAPES:
        add("proximity", want=name)
    for k in range(4):
        for given in itertools.combinations(PROX_SHAPES, k):
            add("proximity", want=(), **{g: z(*PROX_SHAPES[g]) for g in given})
    add("proximity", ball=z(*PROX_SHAPES["ball"]), want=("pairs", "ball"))
    for want in ("Ground", "gap", ("ground", "balls"), ["bogus"], ""):
        add("proximity", want=want)
    add("proximity", want=()); add("proximity", want=[])
    for arg, shape in PROX_SHAPES.items():
        add_wrong("proximity", arg, shape, want=())
    add("proximity", want="bogus", ground=z(N, 22, 3))                             # the order of the checks
    add("proximity", want=(), ground=z(*PROX_SHAPES["ground"], dtype=torch.float64), pairs=z(N, 28, 7))
    add("proximity")
    return t


def parser_table():
    """[(function of bez_isaacgym_amd.abi, args)]: the enum parsers and parameter builders on their own"""
    t = [("body_force_space", (v,)) for v in SPACES + BAD_SPACES]
    t += [("ik_space", (v,)) for v in IK_SPACES + BAD_IK_SPACES]
    t += [("generalized_force_space", (s, at)) for s in SPACES[:4] for at in ATS] + [("generalized_force_space", (0, at)) for at in BAD_ATS]
    t += [("generalized_force_space", (s,)) for s in (0, "local", "world", 2)] + [("generalized_force_space", ("world", "centre"))]
    actuator, dynamics = ("dof_force", "drive_torque", "status"), ("jacobian", "mass_matrix")
    bad = ("torque", "", 3, 2, -1, 1.0, None, True, False)
    t += [("actuator_tensor_id", (v,)) for v in (0, 1, 2) + sum((mixed_case(k) for k in actuator), ()) + bad]
    t += [("dynamics_tensor_id", (v,)) for v in (0, 1) + sum((mixed_case(k) for k in dynamics), ()) + bad]
    t += [("op_space_params", a) for a in ((), (OFFSETS,), (OFFSETS, True), (None, 1), (3,), (OFFSETS[:4],), (None, None), (None, "yes"))]
    t += [("ik_params", a) for a in ((W_ALL,), (W_ALL, OFFSETS, 0.1, 0.2, 8, "root"), (W_ALL, None, 0.05, 0.0, 1, 1), (None,), (W_ALL, [[0.0] * 2] * 5),
                                     (W_ALL, None, 0.0), (W_ALL, None, 0.05, math.nan), (W_ALL, None, 0.05, 0.0, True), (W_ALL, None, 0.05, 0.0, 1, 2))]
    return t


# ---- the record


def _tensor_text(v):
    if isinstance(v, torch.Tensor):
        return "%s%s%s%s" % (str(v.dtype).replace("torch.", ""), tuple(v.shape), "" if v.is_contiguous() else " strided",
                             "" if v.device.type == "cpu" else " on " + v.device.type)
    if isinstance(v, np.ndarray):
        return "ndarray %s%s" % (v.dtype, v.shape)
    return repr(v)


def _text(v):
    if v is W_ALL or v is OFFSETS:
        return "W_ALL" if v is W_ALL else "OFFSETS"
    if isinstance(v, (torch.Tensor, np.ndarray)):   # the parameter tables (weights, offsets, iters) by value
        small = v.ndim == 0 or (v.ndim == 2 and v.shape[0] == 5 and v.shape[1] <= 3)
        return "%s %s" % (type(v).__name__, v.tolist()) if small and str(getattr(v, "device", "cpu")) == "cpu" else _tensor_text(v)
    if isinstance(v, np.generic):
        return "%s(%s)" % (type(v).__name__, v)
    return repr(v)


def _where(addr, named):
    """"<name>+<byte offset>" of the tensor of `named` (name -> tensor) that holds the address"""
    for name, t in named.items():
        if t.data_ptr() <= addr < t.data_ptr() + max(1, t.numel() * t.element_size()):
            return "%s+%d" % (name, addr - t.data_ptr())
    return "unknown+%d" % addr


def _arg(a, named):
    if a is None or isinstance(a, int):
        return a
    if isinstance(a, C.c_void_p):
        return None if a.value is None else _where(a.value, named)
    if hasattr(a, "_obj"):   # ctypes.byref(struct)
        return "%s %s" % (type(a._obj).__name__, bytes(a._obj).hex())
    return "?" + type(a).__name__


def _returned(r, named):
    if isinstance(r, tuple):
        return [_returned(x, named) for x in r]
    if isinstance(r, torch.Tensor):
        return "%s %s %s" % (_where(r.data_ptr(), named), tuple(r.shape), str(r.dtype).replace("torch.", ""))
    return r


def _scratch_of(sim):
    return {"scratch:" + k: t for k, t in sim.__dict__.get("_buffers", {}).items()}


def run_call(sim, method, kw):
    """one entry of the record: the call on `sim`, what the library saw and what came back, or how it was refused"""
    entry = {"call": "%s(%s)" % (method, ", ".join("%s=%s" % (k, _text(v)) for k, v in kw.items()))}
    before, n_calls = {k: t.data_ptr() for k, t in _scratch_of(sim).items()}, len(sim.lib.calls)
    try:
        r = getattr(sim, method)(**kw)
    except Exception as e:
        entry["refused"] = [type(e).__name__, str(e)]
        if len(sim.lib.calls) != n_calls:   # a refusal leaves the library untouched: anything else is recorded
            entry["library_calls"] = len(sim.lib.calls) - n_calls
        return entry
    scratch = _scratch_of(sim)
    named = dict(scratch)
    named.update((k, v) for k, v in reversed(list(kw.items())) if isinstance(v, torch.Tensor) and v.device.type == "cpu")
    entry["library"] = [[name, [_arg(a, named) for a in args]] for name, args in sim.lib.calls[n_calls:]]
    entry["returned"] = _returned(r, named)
    entry["allocated"] = sorted(k for k in scratch if k not in before)
    entry["moved"] = sorted(k for k, p in before.items() if scratch[k].data_ptr() != p)
    return {k: v for k, v in entry.items() if v != []}   # (nothing allocated, nothing moved: left out)


def _ctype_name(t):
    return None if t is None else t.__name__


def record():
    from bez_isaacgym_amd import abi, sim as sim_module
    rec = {"signatures": [[name, _ctype_name(res), [_ctype_name(a) for a in args]] for name, (res, args) in sim_module.SIGS.items()],
           "parsers": [], "calls": []}
    for fn, args in parser_table():
        entry = {"call": "%s(%s)" % (fn, ", ".join(_text(a) for a in args))}
        try:
            r = getattr(abi, fn)(*args)
            entry["returned"] = "%s %s" % (type(r).__name__, bytes(r).hex()) if isinstance(r, C.Structure) else r
        except Exception as e:
            entry["refused"] = [type(e).__name__, str(e)]
        rec["parsers"].append(entry)
    sims = {}
    for k, (method, ball, kw) in enumerate(call_table()):
        if (method, ball) not in sims:
            sims[method, ball] = bare_sim(ball)
        rec["calls"].append(dict(run_call(sims[method, ball], method, kw), sim="%d bodies" % sims[method, ball].num_bodies))
    failing = bare_sim(rc=-3)   # the library's own refusal reaches the caller with its message
    for method, kw in (("inverse_dynamics", {}), ("proximity", {"want": "ball"}), ("apply_body_forces", {"forces": z(N, NB_BALL, 3)})):
        rec["calls"].append(dict(run_call(failing, method, kw), sim="the library fails"))
    return rec


def line(e):
    """an entry of the record as the one line of text the golden file holds for it"""
    if isinstance(e, list):   # a signature
        return "%s: %s(%s)" % (e[0], e[1], ", ".join(e[2]))
    text = e["call"] + (" [%s]" % e["sim"] if e.get("sim", "22 bodies") != "22 bodies" else "")
    if "refused" in e:
        return "%s !! %s: %s%s" % (text, e["refused"][0], e["refused"][1], " (after %d library calls)" % e["library_calls"] if "library_calls" in e else "")
    for name, args in e.get("library", ()):
        text += " -> %s(%s)" % (name, ", ".join("NULL" if a is None else str(a) for a in args))
    text += " = " + (", ".join(str(r) for r in e["returned"]) if isinstance(e["returned"], list) else str(e["returned"]))
    return text + "".join("; %s %s" % (k, ", ".join(e[k])) for k in ("allocated", "moved") if k in e)


def dumps(rec):
    """the record as the text of the golden file: JSON, {section: [line(entry), ...]}, one entry per line"""
    return "{\n%s\n}" % ",\n".join("%s: [\n%s\n]" % (json.dumps(k), ",\n".join(json.dumps(line(e)) for e in v)) for k, v in rec.items())


QUERIES = ("inverse_dynamics", "forward_dynamics", "operational_space", "centroidal", "body_accelerations", "generalized_forces", "limb_ik",
           "proximity")


def refusals(rec):
    """{method: refused entries} of a record's call table"""
    out = {}
    for e in rec["calls"]:
        if "refused" in e:
            name = e["call"].split("(")[0]
            out[name] = out.get(name, 0) + 1
    return out


def time_queries(batches=7, calls=3000):
    """{method: median over the batches of the host seconds per call}, all-default arguments (scratch outputs) on the fake library"""
    sim = bare_sim()
    kws = {"generalized_forces": dict(forces=z(N, NB_BALL, 3)), "limb_ik": dict(targets=z(N, 5, 7), weights=W_ALL)}
    out = {}
    for method in QUERIES:
        fn, kw = getattr(sim, method), kws.get(method, {})
        for _ in range(calls):
            fn(**kw)
        per = []
        for _ in range(batches):
            sim.lib.calls.clear()
            t0 = time.perf_counter()
            for _ in range(calls):
                fn(**kw)
            per.append((time.perf_counter() - t0) / calls)
        out[method] = sorted(per)[len(per) // 2]
    return out


if __name__ == "__main__":
    import bez_isaacgym_amd
    print("bez_isaacgym_amd: %s" % bez_isaacgym_amd.__file__, file=sys.stderr)
    if "--time" in sys.argv:
        print(json.dumps(time_queries()))
    else:
        print(dumps(record()))
