"""CPU suite of the adaptive Rosenbrock controller with the next call's first trial queued ahead
(schemes.ROW_general._trial, QUEUE_NEXT_TRIAL) on the emulation (tests/emu): the branch that takes a queued step
against the controller that launches every trial itself, against the oracle, and under everything a caller can
do between two calls.  Checks and cases: tests/controller_cases.py; the GPU suite (tests/test_gpu_controller.py)
runs the same ones through the HIP path."""
import pytest

from tests import controller_cases as cc
from tests.emu.build_emu import EmuBackend


@pytest.fixture(scope="module")
def backend():
    return EmuBackend()


@pytest.mark.parametrize("name,tol", sorted(cc.HIT_PAIRS))
def test_hit_branch_equals_plain(name, tol, backend):
    on = cc.check_hit_branch_equals_plain(backend, name, tol)
    assert sum(on.hits) == cc.HIT_PAIRS[name, tol]


@pytest.mark.parametrize("name", ["RODASPR", "ROS3PRL", "ROS3PRw"])
def test_hit_branch_against_oracle(name, backend):
    cc.check_hit_branch_against_oracle(backend, name)


@pytest.mark.parametrize("key,value", [("We", 0.02), ("c", 1.5)])
def test_parameter_changed_in_place(key, value, backend):
    cc.check_parameter_changed_in_place(backend, key, value)


@pytest.mark.parametrize("var,node,value", [("h", 0, 1.05), ("q", -1, 1.2), ("T", 7, 0.3)])
def test_node_written_between_calls(var, node, value, backend):
    cc.check_node_written_between_calls(backend, var, node, value)


@pytest.mark.parametrize("variant", ["plain", "pars", "hook"])
def test_through_simulation(variant, backend):
    hits, calls = cc.check_through_simulation(backend, variant)
    assert (hits, calls) == cc.SIMULATION_HITS[variant]


@pytest.mark.parametrize("write", [False, True])
def test_two_schemes_on_one_stepper(write, backend):
    cc.check_two_schemes_on_one_stepper(backend, write)


def test_rejected_trial_with_speculation(backend):
    cc.check_rejected_trial_with_speculation(backend)


def test_stale_container(backend):
    cc.check_stale_container(backend)
