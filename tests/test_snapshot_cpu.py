"""CPU: the Python side of env snapshots (BezSim.snapshot, sim.Snapshot, SimQueries.save_state / load_state) over the fake library of
tests/binding_record.py -- what save / restore refuse before the library is reached, the pointer order they hand over, the default of
load_state's globals_, that a double close destroys once, that the library's refusal reaches the caller with its message, and that
every bez_snapshot_* name of the header has explicit argtypes."""
import ctypes as C
import os
import re

import pytest
import torch

from bez_isaacgym_amd import abi
from tests.binding_record import FakeLib, N, bare_sim, z

M = 5
SNAP_HANDLE = 0x534e


class SnapLib(FakeLib):
    """FakeLib that also records the bez_snapshot_* entry points, hands out SNAP_HANDLE, and fails only the entry points in `failing`"""

    def __init__(self, failing=(), rc=-1):
        FakeLib.__init__(self, 0)
        self.failing, self.fail_rc = tuple(failing), rc

    def __getattr__(self, name):
        if not name.startswith(("bez_sim_", "bez_snapshot_", "bez_query_state_")):
            raise AttributeError(name)

        def entry(*args):
            self.calls.append((name, args))
            if name in ("bez_snapshot_create", "bez_query_state_create"):
                args[2]._obj.value = SNAP_HANDLE
            return self.fail_rc if name in self.failing else 0
        self.__dict__[name] = entry
        return entry


def make(failing=(), rows=M):
    sim = bare_sim()
    sim.lib = SnapLib(failing)
    return sim, sim.snapshot(rows)


def names(sim):
    return [name for name, _ in sim.lib.calls]


def addr(a):
    return None if a is None else a.value


def ids(n):
    return z(n, dtype=torch.int32)


def test_every_snapshot_entry_point_of_the_header_has_explicit_argtypes():
    from bez_isaacgym_amd.sim import QUERY_STATE_SIGS, SIGS, SNAPSHOT_SIGS
    hdr = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "bez_sim.h")).read()
    declared = set(re.findall(r"\b(bez_snapshot_[a-z_0-9]+)\s*\(", hdr))
    assert declared == set(SNAPSHOT_SIGS) and len(declared) == 6
    for name, (res, args) in SNAPSHOT_SIGS.items():
        assert res is C.c_int and args and all(a is not None for a in args), name
    assert not set(SNAPSHOT_SIGS) & (set(SIGS) | set(QUERY_STATE_SIGS))
    for define, value in (("ENVS", abi.SNAPSHOT_ENVS), ("GLOBALS", abi.SNAPSHOT_GLOBALS), ("HEADER_WORDS", abi.SNAPSHOT_HEADER_WORDS),
                          ("GLOBAL_WORDS", abi.SNAPSHOT_GLOBAL_WORDS), ("LAYOUT", abi.SNAPSHOT_LAYOUT), ("SECTIONS", len(abi.SNAPSHOT_SECTIONS))):
        assert int(re.search(r"#define BEZ_SNAPSHOT_%s (\d+)" % define, hdr).group(1)) == value, define
    assert int(re.search(r"#define BEZ_SNAPSHOT_MAGIC (0x[0-9a-f]+)u", hdr).group(1), 16) == abi.SNAPSHOT_MAGIC


def test_create_rows_are_checked_and_a_double_close_destroys_once():
    from bez_isaacgym_amd.sim import BezSimError
    sim, snap = make()
    (name, args), = sim.lib.calls
    assert name == "bez_snapshot_create" and args[1] == M and snap.snap.value == SNAP_HANDLE and snap.rows == M
    for rows in (0, -1, 2.0, None, True, "3"):
        with pytest.raises(BezSimError, match="rows must be an int >= 1"):
            sim.snapshot(rows)
    assert len(sim.lib.calls) == 1
    snap.close()
    assert sim.lib.calls[-1][0] == "bez_snapshot_destroy" and addr(sim.lib.calls[-1][1][1]) == SNAP_HANDLE
    snap.close()
    assert names(sim).count("bez_snapshot_destroy") == 1
    with pytest.raises(BezSimError, match="closed"):
        snap.save()
    with sim.snapshot(2) as other:                       # the context manager closes
        assert other.snap is not None
    assert other.snap is None and names(sim).count("bez_snapshot_destroy") == 2


def test_save_and_restore_hand_the_pointers_over_in_the_header_order():
    sim, snap = make()
    e, r = ids(M), ids(M)
    snap.save()
    name, args = sim.lib.calls[-1]
    assert name == "bez_snapshot_save" and addr(args[1]) == SNAP_HANDLE and args[2] is None and args[3] is None
    snap.save(e)
    assert addr(sim.lib.calls[-1][1][2]) == e.data_ptr()
    snap.restore(env_ids=e, row_ids=r)
    name, args = sim.lib.calls[-1]
    assert name == "bez_snapshot_restore" and addr(args[1]) == SNAP_HANDLE
    assert [addr(args[2]), addr(args[3])] == [e.data_ptr(), r.data_ptr()] and args[4:6] == (M, abi.SNAPSHOT_ENVS)
    snap.restore(globals_=True)                          # no ids: two NULLs, count = the snapshot's rows
    args = sim.lib.calls[-1][1]
    assert args[2] is None and args[3] is None and args[4:6] == (M, abi.SNAPSHOT_ENVS | abi.SNAPSHOT_GLOBALS)
    snap.restore(row_ids=ids(9))                         # fan-out: more entries than rows, by row ids
    assert sim.lib.calls[-1][1][4] == 9
    snap.restore(count=2)
    assert sim.lib.calls[-1][1][4] == 2
    other = bare_sim()                                   # another sim as the destination: its handle goes first
    other.lib, other.h = sim.lib, C.c_void_p(77)
    snap.restore(other, env_ids=ids(3))
    args = sim.lib.calls[-1][1]
    assert addr(args[0]) == 77 and addr(args[1]) == SNAP_HANDLE and args[4] == 3


def test_arguments_are_refused_before_the_library():
    from bez_isaacgym_amd.sim import BezSimError
    sim, snap = make()
    before = len(sim.lib.calls)
    bad_ids = (z(M + 1, dtype=torch.int32), z(M, dtype=torch.int64), z(M), [0] * M, torch.zeros(M, dtype=torch.int32, device="meta"),
               z(M, 2, dtype=torch.int32)[:, 0], z(M, 1, dtype=torch.int32))
    for bad in bad_ids:
        with pytest.raises(BezSimError):
            snap.save(bad)
        with pytest.raises(BezSimError):
            snap.restore(env_ids=bad, count=M)
        with pytest.raises(BezSimError):
            snap.restore(row_ids=bad, count=M)
    with pytest.raises(BezSimError, match="expected shape"):
        snap.restore(env_ids=ids(3), row_ids=ids(4))     # the two id lists differ in length
    with pytest.raises(BezSimError, match="exceeds"):
        snap.restore(env_ids=ids(M + 1))                  # row i for i >= rows
    for count in (-1, 1.0, True, "2"):
        with pytest.raises(BezSimError, match="count"):
            snap.restore(count=count)
    with pytest.raises(BezSimError, match="must be a BezSim"):
        snap.restore(sim=object())
    with pytest.raises(BezSimError, match="int32 CPU tensor"):
        snap.load_state_dict({"header": z(abi.SNAPSHOT_HEADER_WORDS)})
    assert len(sim.lib.calls) == before


def test_a_failing_restore_raises_with_the_librarys_message():
    from bez_isaacgym_amd.sim import BezSimError
    sim, snap = make(failing=("bez_snapshot_restore",))
    with pytest.raises(BezSimError, match=r"failed \(-1\): the fake library was told to fail"):
        snap.restore()
    assert names(sim)[-1] == "bez_snapshot_restore"


def task_over(sim):
    from bez_isaacgym_amd.tasks.base.sim_queries import SimQueries
    task = SimQueries.__new__(SimQueries)
    task.sim, task.num_envs = sim, sim.num_envs
    return task


def what_of(sim):
    name, args = sim.lib.calls[-1]
    assert name == "bez_snapshot_restore"
    return args[5]


def test_load_state_defaults_globals_to_the_whole_sim_identity():
    sim = bare_sim()
    sim.lib = SnapLib()
    task = task_over(sim)
    whole = task.save_state()
    assert whole.rows == N and names(sim)[-2:] == ["bez_snapshot_create", "bez_snapshot_save"]
    both = abi.SNAPSHOT_ENVS | abi.SNAPSHOT_GLOBALS
    task.load_state(whole)
    assert what_of(sim) == both and task._stale is True
    task.load_state(whole, env_ids=ids(N))                # ids given: a partial restore, whatever they hold
    assert what_of(sim) == abi.SNAPSHOT_ENVS
    task.load_state(whole, row_ids=ids(N))
    assert what_of(sim) == abi.SNAPSHOT_ENVS
    task.load_state(whole, globals_=False)
    assert what_of(sim) == abi.SNAPSHOT_ENVS
    task.load_state(whole, env_ids=ids(N), globals_=True)
    assert what_of(sim) == both
    part = task.save_state(ids(2))                        # fewer rows than envs: never the whole sim
    assert part.rows == 2 and addr(sim.lib.calls[-1][1][2]) is not None
    task.load_state(part, env_ids=ids(2))
    assert what_of(sim) == abi.SNAPSHOT_ENVS


def test_load_state_puts_the_host_state_back_only_for_the_whole_sim():
    sim = bare_sim()
    sim.lib = SnapLib()
    task = task_over(sim)
    task.last_step, task.last_rand_step, task.actions = 7, 5, torch.ones(N, 18)
    snap = task.save_state()
    task.last_step, task.last_rand_step, task.actions = 9, 9, torch.zeros(N, 18)
    task.load_state(snap, env_ids=ids(N))
    assert (task.last_step, task.last_rand_step) == (9, 9) and not task.actions.any()
    task.load_state(snap)
    assert (task.last_step, task.last_rand_step) == (7, 5) and bool((task.actions == 1).all())


def test_a_query_state_refuses_save_and_load_state():
    sim = bare_sim()
    sim.lib, sim.cfg = SnapLib(), abi.default_config(N)
    sq = task_over(sim).query_state(M)
    for ask in (sq.save_state, lambda: sq.load_state(None)):
        with pytest.raises(AttributeError, match="query state"):
            ask()
