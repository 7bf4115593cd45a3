"""GPU suite of the write-once node-independent Jacobian planes (tests/uniform_planes_cases.py) through
libtriflow_hip.so and the gfx950 code objects: the sweep kernels' two forms, and captured steps."""
import pytest

from tests import uniform_planes_cases as uc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", uc.TABLE_CASES, ids=lambda c: c[0])
def test_table_equality(case):
    uc.check_table_equality(None, case)


def test_table_equality_large():
    """Sizes with the 8-node sweep segments and the re-spiked level 1 (above 2e6 nodes in all)."""
    uc.check_table_equality(None, ("film_ros2_large", 3, "ROS2", None, 260001, 8, True, ("c", "We")))


def test_invalidation_by_uploads():
    uc.check_invalidation_by_uploads(None)


def test_invalidation_restart():
    uc.check_invalidation_restart(None)


def test_nonuniform_models():
    uc.check_nonuniform_models(None)


def test_rescue_path():
    uc.check_rescue_path(None)


@pytest.mark.parametrize("N", [2000, 50000])
def test_graph_replay(N):
    uc.check_graph_replay(None, N=N)


def test_step_doubling_trial():
    uc.check_step_doubling_trial(None)
