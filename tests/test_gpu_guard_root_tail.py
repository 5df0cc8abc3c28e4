"""The lane-group kernel tests the root / ball part of the non-finite guard in front of the last barrier, and only the pose-error sum
and the reward behind it.  A non-finite torso velocity on the walk and orient tasks (whose rewards read the goal direction / heading
error) must still trip that env alone -- rew 0, reset_buf 1, the same progress / timeout as a twin sim without the fault, its counter
and the health bit -- and the next step must perform the ordinary reset.  The twin check is the one of tests/test_gpu_nonfinite_guard.py."""
import pytest

from bez_isaacgym_amd import abi
from tests.guard_util import _twin

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("value", [float("nan"), float("inf")], ids=["nan", "inf"])
@pytest.mark.parametrize("task", [abi.TASK_WALK, abi.TASK_ORIENT], ids=["walk", "orient"])
@pytest.mark.parametrize("kernel", ["ws8q", "ws8"])
def test_twin_root_trip_goal_tasks(monkeypatch, kernel, task, value):
    _twin(monkeypatch, 64, 40, kernel, task=task, what="root", value=value)


@pytest.mark.parametrize("task", [abi.TASK_KICK, abi.TASK_WALK, abi.TASK_ORIENT], ids=["kick", "walk", "orient"])
def test_twin_root_trip_partial_workgroup(monkeypatch, task):
    # 100 envs: the last workgroup of the lane-group kernel holds 4 envs, and the tripped env is its last one
    _twin(monkeypatch, 100, 99, "ws8q", task=task, what="root", value=float("-inf"))
