"""CPU suite of the explicit Runge-Kutta schemes (schemes.ERK_general, SSPRK3 / RK4 / BS23 / DOPRI5;
tf_step_erk) on the emulation (tests/emu), which runs the unfused form of the step: stage sweeps, tfk_vec and
tfk_vec_maxabs.  Checks and cases: tests/erk_cases.py; the GPU suite (tests/test_gpu_erk.py) runs the same
ones through the HIP path, fused last stage included."""
import numpy as np
import pytest

from tests import erk_cases as ec
from tests.emu.build_emu import EmuBackend
from triflow_amd import schemes
from triflow_amd.tableaux import ERK_TABLEAUX


@pytest.fixture(scope="module")
def backend():
    return EmuBackend()


def test_tableaux_are_consistent():
    """Row sums of b and b_err are one, a is strictly lower triangular, c = row sums of a lie in [0, 1]."""
    for name, tab in ERK_TABLEAUX.items():
        assert abs(tab.b.sum() - 1) < 1e-15 and np.all(np.triu(tab.a) == 0), name
        if tab.b_err is not None:
            assert abs(tab.b_err.sum() - 1) < 1e-15, name
            assert np.array_equal(tab.a[-1], tab.b)         # first same as last
        c = tab.a.sum(axis=1)
        assert c[0] == 0 and (c >= 0).all() and (c <= 1 + 1e-15).all(), name
        # order conditions up to three: sum b c = 1/2, sum b c^2 = 1/3, sum b (a c) = 1/6
        assert abs(tab.b @ c - 1 / 2) < 1e-15 and abs(tab.b @ c ** 2 - 1 / 3) < 1e-15, name
        assert abs(tab.b @ (tab.a @ c) - 1 / 6) < 1e-15, name
    assert set(ec.TABLEAUX) == set(ERK_TABLEAUX)
    for name in ec.TABLEAUX:
        assert name in schemes.__all__ and issubclass(getattr(schemes, name), schemes.ERK_general)


@pytest.mark.parametrize("periodic", [True, False])
@pytest.mark.parametrize("N", ec.SHAPES)
@pytest.mark.parametrize("case", sorted(ec.CASES))
def test_bits_against_numpy(case, N, periodic, backend):
    ec.check_bits_against_numpy(backend, case, N, periodic)


@pytest.mark.parametrize("periodic", [True, False])
@pytest.mark.parametrize("which", sorted(ec.HOOKS))
def test_hook_bits(which, periodic, backend):
    ec.check_hook_bits(backend, which, 203, periodic)


def test_step_by_step_equals_numpy_on_the_raw_solver(backend):
    ec.check_graph_run_against_numpy(backend)


def test_nan_wins(backend):
    ec.check_nan_wins(backend)


def test_zero_coefficient_rule(backend):
    ec.check_zero_coefficient_rule(backend)


def test_window_term_outside_the_update(backend):
    ec.check_window_term_outside_the_update(backend)
    info = ec.raw_solver(backend, "upwind_exact", 203, False)[0].erk_info()
    assert not info["fused"] and info["steps"] >= ec.NSTEPS and info["fused_steps"] == 0     # the emulation


@pytest.mark.parametrize("tab_name", ec.TABLEAUX)
def test_order(tab_name, backend):
    ec.check_order(backend, tab_name)


@pytest.mark.parametrize("tab_name", ["BS23", "DOPRI5"])
def test_controller(tab_name, backend):
    ec.check_controller(backend, tab_name)


@pytest.mark.parametrize("tab_name", ["BS23", "DOPRI5"])
def test_controller_rejects(tab_name, backend):
    """The internal dt starts far too large: the first trials are rejected."""
    _, rejected = ec.check_controller(backend, tab_name, ncalls=3, call_dt=50.0, start=50.0)
    assert rejected >= 1


def test_controller_limits(backend):
    ec.check_controller_limits(backend)


def test_step_factor_of_the_rosenbrock_classes_is_the_square_root(backend):
    """The one refactored method: ROW_general keeps sqrt(tol / err), ERK_general takes the order's root."""
    m = ec.device_model("advdiff", backend)
    row, erk = schemes.ROS3PRw(m, tol=1e-3), schemes.DOPRI5(m, tol=1e-3)
    row._err = erk._err = np.float64(3.7e-5)
    assert row._step_factor() == np.sqrt(1e-3 / np.float64(3.7e-5))
    assert erk._step_factor() == (1e-3 / np.float64(3.7e-5)) ** (1 / 5)
    assert erk.QUEUE_NEXT_TRIAL is False and row.QUEUE_NEXT_TRIAL is True


def test_simulation_fixed(backend):
    ec.check_simulation_fixed(backend, with_probe=False)


def test_simulation_step_doubling(backend):
    ec.check_simulation_step_doubling(backend)


@pytest.mark.parametrize("scheme", ["RK4", "SSPRK3"])
def test_ensemble(scheme, backend):
    ec.check_ensemble(backend, scheme)


def test_no_factorisation(backend):
    ec.check_no_factorisation(backend)


def test_bad_tableaux_are_refused(backend):
    m = ec.device_model("advdiff", backend)
    from triflow_amd.ensemble import Ensemble
    x = np.linspace(0, 1, 16, endpoint=False)
    assert Ensemble(m, x, dict(U=np.ones((1, 16))), dict(k=1e-3, c=0.03), True, scheme="DOPRI5").erk is None
    with pytest.raises(ValueError):
        schemes.ERK_general(m, [[0, 1], [1, 0]], [0.5, 0.5])
    with pytest.raises(ValueError):
        schemes.ERK_general(m, np.zeros((9, 9)), np.ones(9) / 9)
    with pytest.raises(ValueError):
        schemes.ERK_general(m, [[0, 0], [1, 0]], [0.5, 0.5], time_stepping=True, tol=1e-3)
    solver, fd, pars, dt = ec.raw_solver(backend, "advdiff", 7, True)
    with pytest.raises(RuntimeError):
        solver.step_erk(0, 0, dt, [[0, 0], [1, 0]], [0.5, 0.5])                 # src == dst
    with pytest.raises(RuntimeError):
        solver.step_erk(0, 1, dt, [[0, 0], [1, 0]], [0.0, 0.0])                 # no weight
    with pytest.raises(RuntimeError):
        solver.step_erk(0, 1, dt, [[0, 0], [1, 0.5]], [0.5, 0.5])               # a_11 != 0
