"""GPU suite of the explicit Runge-Kutta schemes (tests/erk_cases.py) through libtriflow_hip.so and the gfx950
code objects: the fused last stage (tfk_sweep_f_erk_last / _n, the default) against the NumPy restatement, against
the unfused form (``TRIFLOW_ERK_FUSED=0``, a child process: the switch is read when a solver is created) and
under HIP-graph replay.  The CPU suite (tests/test_erk.py) runs the shared checks on the emulation."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import erk_cases as ec

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("periodic", [True, False])
@pytest.mark.parametrize("N", ec.SHAPES)
@pytest.mark.parametrize("case", sorted(ec.CASES))
def test_bits_against_numpy(case, N, periodic):
    ec.check_bits_against_numpy(None, case, N, periodic)


@pytest.mark.parametrize("periodic", [True, False])
@pytest.mark.parametrize("which", sorted(ec.HOOKS))
def test_hook_bits(which, periodic):
    ec.check_hook_bits(None, which, 203, periodic)


def _child(tmp, name, mode, **env):
    path = os.path.join(str(tmp), name + ".npz")
    full = dict(os.environ)
    for key in ("TRIFLOW_ERK_FUSED", "TRIFLOW_GRAPHS"):
        full.pop(key, None)
    full.update(env)
    subprocess.run([sys.executable, "-m", "tests.erk_cases", mode, path], cwd=ROOT, env=full, check=True,
                   timeout=600)
    with np.load(path) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def dumps(tmp_path_factory):
    """Every case of erk_cases.dump in two fresh processes: the default (fused) and TRIFLOW_ERK_FUSED=0."""
    tmp = tmp_path_factory.mktemp("erk")
    return _child(tmp, "fused", "dump"), _child(tmp, "unfused", "dump", TRIFLOW_ERK_FUSED="0")


@pytest.mark.parametrize("case", sorted(ec.CASES) + ["hook", "graph", "nan", "zero", "heun"])
def test_fused_equals_unfused(case, dumps):
    """(2) States and estimates bit-identical at every shape; NaNs in the same places."""
    fused, unfused = dumps
    assert sorted(fused) == sorted(unfused)
    keys = [k for k in fused if k.split("|")[0] == case]
    assert keys and (case not in ec.CASES or len(keys) == 6 * len(ec.SHAPES) * 2)   # 4 states + 2 estimates
    for k in keys:
        assert np.array_equal(fused[k], unfused[k], equal_nan=True), k
        assert np.isfinite(fused[k]).all() or case == "nan", k


def test_the_two_children_ran_the_two_forms(dumps):
    """(2) The default child took every explicit step with the fused last stage, the other child none: what
    ``tf_erk_info`` says of a raw solver and of a stepper's solver in each (fused, steps, fused steps)."""
    fused, unfused = dumps
    for key in ("info|raw", "info|stepper"):
        f, steps, fused_steps = fused[key]
        assert f == 1 and steps > 0 and fused_steps == steps, (key, fused[key])
        f, steps, fused_steps = unfused[key]
        assert f == 0 and steps > 0 and fused_steps == 0, (key, unfused[key])
        assert fused[key][1] == unfused[key][1]


def test_window_term_outside_the_update():
    ec.check_window_term_outside_the_update(None)
    assert ec.raw_solver(None, "upwind_exact", 203, False)[0].erk_info()["fused"]


def test_graph_replay(tmp_path):
    """(3) N = 203 with TRIFLOW_GRAPHS=1 and =0, ten steps at one dt and three at another: bit-identical, and
    every step's estimate is its own (the yardstick's for that step, all thirteen distinct)."""
    on = _child(tmp_path, "graphs_on", "dump_graph", TRIFLOW_GRAPHS="1")
    off = _child(tmp_path, "graphs_off", "dump_graph", TRIFLOW_GRAPHS="0")
    for k in ("graph|U", "graph|err"):
        assert np.array_equal(on[k], off[k]), k
    states, errs = ec.check_graph_run_against_numpy(None)         # (this process: graphs on by size)
    assert np.array_equal(on["graph|U"], np.array(states)) and np.array_equal(on["graph|err"], np.array(errs))


def test_nan_wins():
    ec.check_nan_wins(None)


def test_zero_coefficient_rule():
    ec.check_zero_coefficient_rule(None)


@pytest.mark.parametrize("tab_name", ["BS23", "DOPRI5"])
def test_controller(tab_name):
    ec.check_controller(None, tab_name)


@pytest.mark.parametrize("tab_name", ["BS23", "DOPRI5"])
def test_controller_rejects(tab_name):
    _, rejected = ec.check_controller(None, tab_name, ncalls=3, call_dt=50.0, start=50.0)
    assert rejected >= 1


def test_controller_limits():
    ec.check_controller_limits(None)


def test_simulation_fixed_with_probe():
    ec.check_simulation_fixed(None, with_probe=True)


def test_simulation_step_doubling():
    ec.check_simulation_step_doubling(None)


@pytest.mark.parametrize("scheme", ["RK4", "SSPRK3"])
def test_ensemble(scheme):
    ec.check_ensemble(None, scheme)


def test_no_factorisation():
    ec.check_no_factorisation(None)
