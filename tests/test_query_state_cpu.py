"""CPU: the Python side of query states (BezSim.query_state, sim.QueryState, SimQueries.query_state) over the fake library of
tests/binding_record.py -- what set / capture refuse before the library is reached and what they hand it, that every query on a query
state runs between a bind and an unbind, also when it fails, that results have the query state's row count, and that the task-level
queries forward to it while the ones about physics launches refuse."""
import ctypes as C

import numpy as np
import pytest
import torch

from bez_isaacgym_amd import abi
from tests.binding_record import FakeLib, N, W_ALL, bare_sim, z

M = 5
QS_HANDLE = 0x5150


class QueryLib(FakeLib):
    """FakeLib that also records the bez_query_state_* entry points, hands out QS_HANDLE, and fails only the entry points in `failing`"""

    def __init__(self, failing=(), rc=-3):
        FakeLib.__init__(self, 0)
        self.failing, self.fail_rc = tuple(failing), rc

    def __getattr__(self, name):
        if not name.startswith(("bez_sim_", "bez_query_state_")):
            raise AttributeError(name)

        def entry(*args):
            self.calls.append((name, args))
            if name == "bez_query_state_create":
                args[2]._obj.value = QS_HANDLE
            return self.fail_rc if name in self.failing else 0
        self.__dict__[name] = entry
        return entry


def make(ball=True, failing=(), rows=M):
    sim = bare_sim(ball)
    sim.lib = QueryLib(failing)
    return sim, sim.query_state(rows)


def names(sim):
    return [name for name, _ in sim.lib.calls]


def addr(a):
    return None if a is None else a.value


def test_create_reaches_the_library_and_rows_are_checked():
    from bez_isaacgym_amd.sim import BezSimError
    sim, qs = make()
    (name, args), = sim.lib.calls
    assert name == "bez_query_state_create" and args[1] == M and qs.qs.value == QS_HANDLE and qs.rows == M
    for rows in (0, -1, 2.0, None, True, "3"):
        with pytest.raises(BezSimError, match="rows must be an int >= 1"):
            sim.query_state(rows)
    assert len(sim.lib.calls) == 1
    qs.close()
    assert sim.lib.calls[-1][0] == "bez_query_state_destroy" and addr(sim.lib.calls[-1][1][1]) == QS_HANDLE
    qs.close()                                        # closing twice destroys once
    assert names(sim).count("bez_query_state_destroy") == 1


def test_set_hands_the_pointers_over_in_the_documented_order():
    sim, qs = make()
    root, dof, ball, ids = z(M, 13), z(M, 18, 2), z(M, 13), z(M, dtype=torch.int32)
    qs.set(root, dof, ball, ids)
    name, args = sim.lib.calls[-1]
    assert name == "bez_query_state_set" and addr(args[1]) == QS_HANDLE
    assert [addr(a) for a in args[2:6]] == [root.data_ptr(), dof.data_ptr(), ball.data_ptr(), ids.data_ptr()] and args[6] is None
    qs.set(root, z(M * 18, 2))                          # the flat DOF_STATE layout; no ball, no ids: two NULLs
    name, args = sim.lib.calls[-1]
    assert [addr(a) for a in args[2:6]][0] == root.data_ptr() and [addr(a) for a in args[4:6]] == [None, None]
    qs.capture(ids)
    name, args = sim.lib.calls[-1]
    assert name == "bez_query_state_capture" and addr(args[1]) == QS_HANDLE and addr(args[2]) == ids.data_ptr()
    assert "bez_query_state_bind" not in names(sim)    # set and capture need no binding


def bad_tensors(shape, dtype=torch.float32):
    other = torch.float64 if dtype == torch.float32 else torch.int64
    return (z(shape[0] + 1, *shape[1:], dtype=dtype), z(*shape[:-1], shape[-1] + 1, dtype=dtype), z(*shape, dtype=other),
            np.zeros(shape, np.float32), torch.zeros(shape, dtype=dtype, device="meta"),
            z(*(shape + (2,)), dtype=dtype)[..., 0], z(N, *shape[1:], dtype=dtype))


@pytest.mark.parametrize("arg,shape,dtype", [("root", (M, 13), torch.float32), ("dof", (M, 18, 2), torch.float32), ("ball", (M, 13), torch.float32),
                                             ("env_ids", (M,), torch.int32)])
def test_set_and_capture_refuse_before_the_library(arg, shape, dtype):
    from bez_isaacgym_amd.sim import BezSimError
    sim, qs = make()
    before = len(sim.lib.calls)
    for bad in bad_tensors(shape, dtype):
        kw = dict(root=z(M, 13), dof=z(M, 18, 2), ball=z(M, 13), env_ids=z(M, dtype=torch.int32))
        kw[arg] = bad
        with pytest.raises(BezSimError):
            qs.set(**kw)
        if arg == "env_ids":
            with pytest.raises(BezSimError):
                qs.capture(bad)
    assert len(sim.lib.calls) == before


def test_ball_and_identity_capture_rules():
    from bez_isaacgym_amd.sim import BezSimError
    sim, qs = make(ball=False)
    before = len(sim.lib.calls)
    with pytest.raises(BezSimError, match="no ball"):
        qs.set(z(M, 13), z(M, 18, 2), ball=z(M, 13))
    with pytest.raises(BezSimError, match="rows == num_envs"):
        qs.capture()                                   # M = 5 rows, N = 3 envs
    assert len(sim.lib.calls) == before
    same = sim.query_state(N)
    same.capture()
    assert sim.lib.calls[-1][0] == "bez_query_state_capture" and addr(sim.lib.calls[-1][1][2]) is None


def query_calls(ball=True):
    """(method, kwargs, the shapes of what it returns) for M rows"""
    nb = 22 if ball else 21
    return [("inverse_dynamics", {}, [(M, 24)]), ("inverse_dynamics", dict(udot=z(M, 24), terms=1), [(M, 24)]),
            ("forward_dynamics", dict(force=z(M, 24), bias=0), [(M, 24)]),
            ("operational_space", {}, [(M, 5, 6, 24), (M, 5, 6, 24), (M, 30, 30), (M, 5, 6, 6)]),
            ("centroidal", dict(want_matrix=True), [(M, 16), (M, 6, 24)]),
            ("body_accelerations", {}, [(M, 21, 6)]),
            ("generalized_forces", dict(forces=z(M, nb, 3)), [(M, 24)]),
            ("limb_ik", dict(targets=z(M, 5, 7), weights=W_ALL), [(M, 18), (M, 5, 6)]),
            ("proximity", {}, [(M, 23, 3), (M, 11, 8), (M, 28, 8)])]


@pytest.mark.parametrize("method,kw,shapes", query_calls())
def test_every_query_binds_calls_unbinds_and_returns_m_rows(method, kw, shapes):
    sim, qs = make()
    before = len(sim.lib.calls)
    r = getattr(qs, method)(**kw)
    r = r if isinstance(r, tuple) else (r,)
    assert [tuple(t.shape) for t in r] == shapes
    (b, bargs), (q, qargs), (u, uargs) = sim.lib.calls[before:]
    assert (b, q, u) == ("bez_query_state_bind", "bez_sim_" + method, "bez_query_state_bind")
    assert addr(bargs[1]) == QS_HANDLE and uargs[1] is None
    # its own buffers, not the sim's: the sim's same call allocates N-row ones and leaves these alone
    assert "_buffers" not in sim.__dict__
    mine = {k: t.data_ptr() for k, t in qs._buffers.items()}
    live_kw = {k: (z(N, *v.shape[1:]) if isinstance(v, torch.Tensor) else v) for k, v in kw.items()}
    live = getattr(sim, method)(**live_kw)
    live = live if isinstance(live, tuple) else (live,)
    assert all(t.shape[0] == N for t in live) and sim.lib.calls[-1][0] == "bez_sim_" + method and sim.lib.calls[-2][0] == "bez_query_state_bind"
    assert {k: t.data_ptr() for k, t in qs._buffers.items()} == mine


@pytest.mark.parametrize("method,kw,shapes", query_calls())
def test_a_failing_query_raises_and_still_unbinds(method, kw, shapes):
    from bez_isaacgym_amd.sim import BezSimError
    sim, qs = make(failing=("bez_sim_" + method,))
    before = len(sim.lib.calls)
    with pytest.raises(BezSimError, match=r"failed \(-3\)"):
        getattr(qs, method)(**kw)
    assert names(sim)[before:] == ["bez_query_state_bind", "bez_sim_" + method, "bez_query_state_bind"]
    assert addr(sim.lib.calls[before][1][1]) == QS_HANDLE and sim.lib.calls[-1][1][1] is None


def test_a_failing_bind_never_runs_the_query_on_the_live_state():
    from bez_isaacgym_amd.sim import BezSimError
    sim, qs = make(failing=("bez_query_state_bind",))
    with pytest.raises(BezSimError):
        qs.inverse_dynamics()
    assert "bez_sim_inverse_dynamics" not in names(sim)


def test_wrong_row_counts_are_refused_against_m():
    from bez_isaacgym_amd.sim import BezSimError
    sim, qs = make()
    before = len(sim.lib.calls)
    for call in (lambda: qs.inverse_dynamics(udot=z(N, 24)), lambda: qs.forward_dynamics(out=z(N, 24)), lambda: qs.centroidal(state=z(N, 16)),
                 lambda: qs.limb_ik(z(N, 5, 7), W_ALL), lambda: qs.proximity(ground=z(N, 23, 3), want=()),
                 lambda: qs.generalized_forces(forces=z(N, 22, 3)), lambda: qs.operational_space(jac=z(N, 5, 6, 24), want=())):
        with pytest.raises(BezSimError, match="expected shape"):
            call()
    assert len(sim.lib.calls) == before


def test_tensors_and_refreshes_reach_the_query_state_entry_points():
    from bez_isaacgym_amd.sim import BezSimError
    sim, qs = make()
    qs._wrap = lambda key, getter, which: (getter(qs.h, which, None, None, None, None), ("view", which))[1]   # no device: record the getter's call
    assert qs.dynamics_tensor("jacobian") == ("view", abi.QUERY_JACOBIAN)
    name, args = sim.lib.calls[-1]
    assert name == "bez_query_state_tensor" and addr(args[1]) == QS_HANDLE and args[2] == abi.QUERY_JACOBIAN
    qs.refresh_dynamics_tensors(("jacobian", "mass_matrix"))
    name, args = sim.lib.calls[-1]
    assert name == "bez_query_state_refresh" and args[2] == (1 << abi.QUERY_JACOBIAN) | (1 << abi.QUERY_MASS_MATRIX)
    assert qs.refresh(abi.TENSOR_RIGID_BODY_STATE) == ("view", abi.QUERY_RIGID_BODY_STATE)
    assert sim.lib.calls[-1][0] == "bez_query_state_refresh" and sim.lib.calls[-1][1][2] == 1 << abi.QUERY_RIGID_BODY_STATE
    with pytest.raises(BezSimError, match="TENSOR_RIGID_BODY_STATE only"):
        qs.refresh(abi.TENSOR_DOF_STATE)
    assert "bez_query_state_bind" not in names(sim)


def task_over(sim):
    from bez_isaacgym_amd.tasks.base.sim_queries import SimQueries
    task = SimQueries.__new__(SimQueries)
    task.sim, task.num_envs = sim, sim.num_envs
    return task


def test_sim_queries_over_a_query_state_forward_to_it():
    from bez_isaacgym_amd.tasks.base.sim_queries import SimQueries
    sim = bare_sim()
    sim.lib, sim.cfg = QueryLib(), abi.default_config(N)
    task = task_over(sim)
    assert task.query_state().num_envs == N             # rows=None: num_envs
    sq = task.query_state(M)
    assert isinstance(sq, SimQueries) and sq.num_envs == M and sq.sim.rows == M
    sq.set(z(M, 13), z(M, 18, 2))
    assert sim.lib.calls[-1][0] == "bez_query_state_set"
    for call, entry, shape in ((sq.gravity_forces, "bez_sim_inverse_dynamics", (M, 24)), (sq.foot_clearance, "bez_sim_proximity", (M, 2)),
                               (lambda: sq.center_of_mass()[0], "bez_sim_centroidal", (M, 3)),
                               (sq.end_effector_jacobian, "bez_sim_operational_space", (M, 5, 6, 24))):
        before = len(sim.lib.calls)
        assert tuple(call().shape) == shape
        assert names(sim)[before:] == ["bez_query_state_bind", entry, "bez_query_state_bind"]
    assert "_buffers" not in sim.__dict__               # nothing landed in the sim's own result buffers
    sq.close()
    assert sim.lib.calls[-1][0] == "bez_query_state_destroy"


def test_what_is_about_physics_launches_refuses_on_a_query_state():
    sim = bare_sim()
    sim.lib, sim.cfg = QueryLib(), abi.default_config(N)
    sq = task_over(sim).query_state(M)
    before = len(sim.lib.calls)
    for ask in (lambda: sq.dof_force_tensor, sq.refresh_dof_force_tensor, sq.actuator_snapshot,
                lambda: sq.apply_rigid_body_force_tensors(forces=z(M, 22, 3)), lambda: sq.apply_rigid_body_force_at_pos_tensors(z(M, 22, 3))):
        with pytest.raises(AttributeError, match="query state"):
            ask()
    assert len(sim.lib.calls) == before
