"""GPU suite of the adaptive Rosenbrock controller with the next call's first trial queued ahead
(tests/controller_cases.py) through libtriflow_hip.so and the gfx950 code objects.  The CPU suite
(tests/test_controller.py) runs the same checks on the emulation."""
import pytest

from tests import controller_cases as cc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name,tol", sorted(cc.HIT_PAIRS))
def test_hit_branch_equals_plain(name, tol):
    cc.check_hit_branch_equals_plain(None, name, tol)


@pytest.mark.parametrize("name", ["RODASPR", "ROS3PRL", "ROS3PRw"])
def test_hit_branch_against_oracle(name):
    cc.check_hit_branch_against_oracle(None, name)


@pytest.mark.parametrize("key,value", [("We", 0.02), ("c", 1.5)])
def test_parameter_changed_in_place(key, value):
    cc.check_parameter_changed_in_place(None, key, value)


@pytest.mark.parametrize("var,node,value", [("h", 0, 1.05), ("q", -1, 1.2), ("T", 7, 0.3)])
def test_node_written_between_calls(var, node, value):
    cc.check_node_written_between_calls(None, var, node, value)


@pytest.mark.parametrize("variant", ["plain", "pars", "hook"])
def test_through_simulation(variant):
    hits, calls = cc.check_through_simulation(None, variant)
    assert (hits == 0) if variant == "hook" else (hits > calls // 2), (hits, calls)


@pytest.mark.parametrize("write", [False, True])
def test_two_schemes_on_one_stepper(write):
    cc.check_two_schemes_on_one_stepper(None, write)


def test_rejected_trial_with_speculation():
    cc.check_rejected_trial_with_speculation(None)


def test_stale_container():
    cc.check_stale_container(None)
