"""Checks of the explicit Runge-Kutta schemes (schemes.ERK_general, SSPRK3 / RK4 / BS23 / DOPRI5; tf_step_erk),
shared by the CPU suite (tests/test_erk.py: the emulation, which runs the unfused form -- stage sweeps, tfk_vec,
tfk_vec_maxabs) and the GPU suite (tests/test_gpu_erk.py: the HIP path, fused last stage by default).

The yardstick is :func:`numpy_step`, a NumPy restatement of the arithmetic contract of ``tf_step_erk``
(include/triflow_hip.h) that never calls the code under test::

    k_i  = dt * F(U + (((a_i0*k_0) + a_i1*k_1) + ...))
    U+   = U + (((b_0*k_0) + b_1*k_1) + ...)
    err  = max |((d_0*k_0) + d_1*k_1) + ...|,  d = b - b_err;  NaN wins

with the exactly-zero coefficients left out of every sum.  Its F is ``oracle.numpy_path.compute_F`` on the
model's own SymPy arrays (``Heaviside = numpy.heaviside`` for the model built with ``heaviside="exact"``), which
the project's F equals bit for bit (tests/parity_cases.py, tests/heaviside_cases.py).

Run as a program (``python -m tests.erk_cases dump <file.npz>``) it writes the states and estimates of every
case of :func:`dump_cases`: the GPU suite starts it twice, with ``TRIFLOW_ERK_FUSED=0`` and without, because
the switch is read when a solver is created.
"""
import gc
import sys
from functools import lru_cache, partial

import numpy as np
from sympy import lambdify

from oracle import corpus, numpy_path as ora
from triflow_amd import Model, Simulation, schemes
from triflow_amd.compilers import hip_compiler
from triflow_amd.device import DirichletHook
from triflow_amd.ensemble import Ensemble
from triflow_amd.schemes import null_hook
from triflow_amd.tableaux import ERK_TABLEAUX

TABLEAUX = ("SSPRK3", "RK4", "BS23", "DOPRI5")
#: one chunk; ragged, several chunks and segments; more than one workgroup of 64 chunks with a ragged tail
SHAPES = (7, 203, 4099)
#: case -> (corpus model, heaviside mode, per-node parameters, dt): dt small enough that five steps stay
#: finite on every grid (the film model: the test is about bits, not physics)
CASES = {
    "advdiff": ("M1_advdiff", None, False, 1e-4),
    "upwind_exact": ("upwind2_state", "exact", False, 1e-4),
    "film": ("M3_film", None, False, 1e-9),
    "helper": ("helper", None, False, 1e-6),
    "advdiff_pernode": ("M1_advdiff", None, True, 1e-4),
}
NSTEPS = 5
_EXACT = {"Heaviside": np.heaviside, "DiracDelta": lambda a, *_: np.zeros_like(a)}


# ---------------------------------------------------------------------------------------- models and inputs
@lru_cache(maxsize=None)
def device_model(case, backend):
    name, mode, _, _ = CASES[case]
    eqs, dep, pars, helps = corpus.model_args(name)
    compiler = hip_compiler if backend is None else partial(hip_compiler, backend=backend)
    kw = {} if mode is None else dict(heaviside=mode)
    return Model(eqs, dep, pars, helps, compiler=compiler, **kw)


@lru_cache(maxsize=None)
def _symbolic_model(case):
    name, mode, _, _ = CASES[case]
    eqs, dep, pars, helps = corpus.model_args(name)
    kw = {} if mode is None else dict(heaviside=mode)
    m = Model(eqs, dep, pars, helps, hold_compilation=True, **kw)
    modules = ora._lambdify_modules()
    if mode == "exact":
        modules = [dict(modules[0], **_EXACT), "numpy"]
    return m, lambdify(m._symbolic_args, m.F_array.tolist(), modules=modules)


def inputs(case, N, periodic):
    """(fields dict with x, parameter dict, dt)."""
    name, _, per_node, dt = CASES[case]
    fd = corpus.synthetic_fields(name, N, seed=N, periodic=periodic)
    pars = corpus.synthetic_pars(name, N, periodic, per_node=per_node)
    return fd, pars, dt


def numpy_F(case, fd, pars):
    """U flat [node * nvar + var] -> F flat, the oracle's arithmetic."""
    m, f_func = _symbolic_model(case)
    x, N, nvar = np.asarray(fd["x"]), np.asarray(fd["x"]).size, len(m._dep_vars)
    helps = [np.asarray(fd[h]) for h in m._help_funcs]
    pv = [pars[p] for p in m._pars]

    def F(U):
        cols = np.ascontiguousarray(U.reshape(N, nvar).T)
        with np.errstate(all="ignore"):
            return ora.compute_F(m, f_func, x, *cols, *helps, *pv, pars["periodic"], faithful_interleave=False)
    return F


def flat_state(case, fd):
    m, _ = _symbolic_model(case)
    return np.ascontiguousarray(np.array([fd[k] for k in m._dep_vars], dtype=float).T).reshape(-1)


# ---------------------------------------------------------------------------------------------- the yardstick
def _left_sum(coefs, ks):
    """((c_0*k_0) + c_1*k_1) + ... over the non-zero coefficients; None when there is none."""
    acc = None
    for c, k in zip(coefs, ks):
        if c != 0.0:
            acc = c * k if acc is None else acc + c * k
    return acc


def numpy_stages(F, U, dt, a):
    ks = []
    with np.errstate(all="ignore"):
        for i in range(len(a)):
            acc = _left_sum(a[i][:i], ks)
            ks.append(dt * F(U if acc is None else U + acc))
    return ks


def numpy_step(F, U, dt, a, b, d=None):
    """(U+, err) by the contract; err is None without ``d``."""
    ks = numpy_stages(F, U, dt, a)
    with np.errstate(all="ignore"):
        new = U + _left_sum(b, ks)
        if d is None:
            return new, None
        m = np.abs(_left_sum(d, ks))
    return new, (np.float64(np.nan) if np.isnan(m).any() else m.max())


def tableau(name):
    tab = ERK_TABLEAUX[name]
    d = None if tab.b_err is None else tab.b - tab.b_err
    return tab, d


def apply_hook_flat(hook, t, U, dep):
    """A DirichletHook on a flat state (nodes interleaved by variable)."""
    if hook is None:
        return U
    U, nvar = U.copy(), len(dep)
    for var, nodes in hook.values.items():
        for node, value in nodes.items():
            U.reshape(-1, nvar)[node, dep.index(var)] = value(t) if callable(value) else value
    return U


def numpy_run(case, N, periodic, tab_name, hook=None, nsteps=NSTEPS, dt=None, U0=None):
    """(states, estimates) of ``nsteps`` steps; the hook before and after every step, as the schemes do."""
    fd, pars, dt0 = inputs(case, N, periodic)
    dt = dt0 if dt is None else dt
    F, (tab, d) = numpy_F(case, fd, pars), tableau(tab_name)
    dep = list(_symbolic_model(case)[0]._dep_vars)
    U, t, states, errs = (flat_state(case, fd) if U0 is None else U0), 0.0, [], []
    for _ in range(nsteps):
        U, err = numpy_step(F, apply_hook_flat(hook, t, U, dep), dt, tab.a, tab.b, d)
        t = t + dt
        U = apply_hook_flat(hook, t, U, dep)
        states.append(U)
        errs.append(err)
    return states, errs


# ------------------------------------------------------------------------------------------- the device runs
def general(m, tab_name, **kw):
    """The tableau as a fixed-step ERK_general (BS23 and DOPRI5 then still return their estimate)."""
    tab = ERK_TABLEAUX[tab_name]
    return schemes.ERK_general(m, tab.a, tab.b, b_err=tab.b_err, order=tab.order, **kw)


def device_run(backend, case, N, periodic, tab_name, hook=None, nsteps=NSTEPS, dt=None):
    gc.collect()
    fd, pars, dt0 = inputs(case, N, periodic)
    dt = dt0 if dt is None else dt
    m = device_model(case, backend)
    sch = general(m, tab_name)
    f, t, states, errs = m.fields_template(**fd), 0.0, [], []
    with np.errstate(all="ignore"):
        for _ in range(nsteps):
            t, f, err = sch._fixed_step(t, f, dt, pars, hook=null_hook if hook is None else hook, hook_after=True)
            states.append(f.copy().uflat)
            errs.append(err)
    return states, errs


def same_errs(a, b):
    if a[0] is None or b[0] is None:
        return a[0] is None and b[0] is None
    return np.array_equal(np.array(a, dtype=float), np.array(b, dtype=float), equal_nan=True)


def check_bits_against_numpy(backend, case, N, periodic):
    """(1) Five consecutive steps of each tableau: the states and the estimates of BS23 and DOPRI5."""
    for tab_name in TABLEAUX:
        states, errs = device_run(backend, case, N, periodic, tab_name)
        ref, ref_errs = numpy_run(case, N, periodic, tab_name)
        tag = (case, N, periodic, tab_name)
        assert np.isfinite(ref[-1]).all(), tag
        for k, (x, y) in enumerate(zip(states, ref)):
            assert np.array_equal(x, y), (tag, "step %d" % k, np.abs(x - y).max())
        assert same_errs(errs, ref_errs), (tag, errs, ref_errs)
        if ERK_TABLEAUX[tab_name].b_err is not None:
            assert all(e is not None and e > 0.0 for e in errs), (tag, errs)


HOOKS = {
    "constant": DirichletHook(U={0: 1.0, -1: 0.0}),
    "time": DirichletHook(U={0: lambda t: 1.0 + 100.0 * t, -1: 0.0}),
}


def check_hook_bits(backend, which, N, periodic):
    """(1) ... with a declarative hook, constant and time dependent: applied before and after every step."""
    for tab_name in TABLEAUX:
        states, errs = device_run(backend, "advdiff", N, periodic, tab_name, hook=HOOKS[which])
        ref, ref_errs = numpy_run("advdiff", N, periodic, tab_name, hook=HOOKS[which])
        for k, (x, y) in enumerate(zip(states, ref)):
            assert np.array_equal(x, y), (which, N, periodic, tab_name, k, np.abs(x - y).max())
        assert same_errs(errs, ref_errs), (which, tab_name, errs, ref_errs)
        assert which != "constant" or (states[-1][0] == 1.0 and states[-1][-1] == 0.0)      # the closing hook


# ---------------------------------------------------------------------------- the raw solver (graphs, NaN)
def raw_solver(backend, case, N, periodic):
    """(solver, fields dict, parameter dict, dt): a solver of the model bound to the inputs, state in slot 0."""
    fd, pars, dt = inputs(case, N, periodic)
    m = device_model(case, backend)
    cm = m._device
    values = [pars[k] for k in cm.pars]
    solver = cm.solver(N, periodic, 1, cm.parvec_mask_of(values))
    helps = [np.asarray(fd[h]) for h in m._help_funcs] or None
    cm.bind_inputs(solver, fd["x"], values, helps)
    solver.set_state(0, np.array([fd[k] for k in m._dep_vars]))
    return solver, fd, pars, dt


def solver_state(solver, slot, nvar):
    """[nvar][nsys][N] of a slot -> flat, nodes interleaved by variable (system 0)."""
    return np.ascontiguousarray(np.asarray(solver.get_state(slot))[:, 0, :].T).reshape(-1)


def raw_steps(solver, U_shape, tab_name, dts):
    """Ping-pong between slots 0 and 1; (states, estimates)."""
    tab, d = tableau(tab_name)
    states, errs, src = [], [], 0
    for dt in dts:
        with np.errstate(all="ignore"):
            errs.append(solver.step_erk(src, 1 - src, dt, tab.a, tab.b, d))
        src = 1 - src
        states.append(solver_state(solver, src, U_shape))
    return states, errs


GRAPH_DTS = (1e-4,) * 10 + (7e-5,) * 3


def graph_run(backend, tab_name="DOPRI5"):
    """(3) N = 203, ten steps at one dt and three at another on the raw solver: every (src, dst, dt) comes
    back often enough that, with graphs on, steps are captured and replayed."""
    solver, fd, pars, _ = raw_solver(backend, "advdiff", 203, True)
    return raw_steps(solver, 1, tab_name, GRAPH_DTS)


def check_graph_run_against_numpy(backend, tab_name="DOPRI5"):
    """... against the yardstick: the estimate of every step is that step's own."""
    states, errs = graph_run(backend, tab_name)
    fd, pars, _ = inputs("advdiff", 203, True)
    F, (tab, d) = numpy_F("advdiff", fd, pars), tableau(tab_name)
    U = flat_state("advdiff", fd)
    for k, dt in enumerate(GRAPH_DTS):
        U, err = numpy_step(F, U, dt, tab.a, tab.b, d)
        assert np.array_equal(states[k], U), (tab_name, k)
        assert errs[k] == err, (tab_name, k, errs[k], err)
    assert len(set(errs)) == len(errs)           # no two steps share an estimate: a stale one would show
    return states, errs


def check_nan_wins(backend, N=203):
    """(4) One NaN in U: the estimate is NaN; the state equals the yardstick's, NaNs where it has them."""
    out = {}
    for tab_name in ("BS23", "DOPRI5"):
        solver, fd, pars, dt = raw_solver(backend, "advdiff", N, True)
        U = flat_state("advdiff", fd)
        U[N // 2] = np.nan
        solver.set_state(0, U.reshape(1, 1, N))
        states, errs = raw_steps(solver, 1, tab_name, (dt,))
        tab, d = tableau(tab_name)
        ref, ref_err = numpy_step(numpy_F("advdiff", fd, pars), U, dt, tab.a, tab.b, d)
        assert np.isnan(errs[0]) and np.isnan(ref_err), (tab_name, errs, ref_err)
        assert np.array_equal(states[0], ref, equal_nan=True) and np.isnan(ref).any() and not np.isnan(ref).all()
        out[tab_name] = (states[0], errs[0])
    return out


#: Three stages made to show the rule: stage 1 is F(U + k_0), stage 2 is F(U) again (a_20 = a_21 = 0), and
#: neither the update nor the estimate reads k_1.
ZERO_A = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 0.0]])
ZERO_B = np.array([0.5, 0.0, 0.5])
ZERO_D = np.array([1.0, 0.0, 0.5])
ZERO_DT = 1e200


def check_zero_coefficient_rule(backend, N=203):
    """(4) A non-finite k_j reaches U+ and the estimate only through the sums that contain it.  With RK4
    itself the rule cannot show in U+: where k_0 is not finite, the state of stage 1 (U + k_0/2) is not,
    so k_1 is not either, at the same nodes -- and b_1 k_1 is part of U+; leaving 0 * k_0 out of stage 2
    changes nothing that b_1 k_1 has not already spoilt.  So the rule is tested where it can be seen, on a
    tableau of the same shape (ZERO_A: a_20 = 0 like RK4's, and a_21 = b_1 = d_1 = 0): on the linear
    model M1_advdiff with dt = 1e200, k_0 = dt F(U) is finite (~1e200), k_1 = dt F(U + k_0) overflows to
    +-inf at every node, k_2 = dt F(U) is finite again.  By the contract U+ = U + (k_0/2 + k_2/2) and err =
    max |k_0 + k_2/2| are finite; with the zero coefficients multiplied in, both would be NaN everywhere."""
    solver, fd, pars, _ = raw_solver(backend, "advdiff", N, True)
    U = flat_state("advdiff", fd)
    F = numpy_F("advdiff", fd, pars)
    ks = numpy_stages(F, U, ZERO_DT, ZERO_A)
    assert np.isfinite(ks[0]).all() and np.isinf(ks[1]).all() and np.array_equal(ks[2], ks[0])
    with np.errstate(all="ignore"):
        err = solver.step_erk(0, 1, ZERO_DT, ZERO_A, ZERO_B, ZERO_D)
        got = solver_state(solver, 1, 1)
        ref, ref_err = numpy_step(F, U, ZERO_DT, ZERO_A, ZERO_B, ZERO_D)
        literal = U + ((ZERO_B[0] * ks[0] + ZERO_B[1] * ks[1]) + ZERO_B[2] * ks[2])
    assert np.isfinite(ref).all() and np.isfinite(ref_err) and np.isnan(literal).all()
    assert np.array_equal(got, ref) and err == ref_err, (err, ref_err)
    return np.append(got, err)


#: Heun's third-order scheme: k_1 is part of the last stage's state (a_21 = 2/3) but not of the update
#: (b_1 = 0) -- a term the fused last stage holds in its window and leaves out of the sum; none of the four
#: named tableaux has one.  With an estimate against the embedded Euler step (d = b - (1, 0, 0)).
HEUN_A = np.array([[0.0, 0.0, 0.0], [1 / 3, 0.0, 0.0], [0.0, 2 / 3, 0.0]])
HEUN_B = np.array([1 / 4, 0.0, 3 / 4])
HEUN_D = HEUN_B - np.array([1.0, 0.0, 0.0])


def check_window_term_outside_the_update(backend, case="upwind_exact", N=203, periodic=False):
    """Five steps of Heun's scheme on the raw solver against the yardstick, states and estimates."""
    solver, fd, pars, dt = raw_solver(backend, case, N, periodic)
    F, U = numpy_F(case, fd, pars), flat_state(case, fd)
    nvar, src, out = len(_symbolic_model(case)[0]._dep_vars), 0, []
    for k in range(NSTEPS):
        err = solver.step_erk(src, 1 - src, dt, HEUN_A, HEUN_B, HEUN_D)
        src = 1 - src
        U, ref_err = numpy_step(F, U, dt, HEUN_A, HEUN_B, HEUN_D)
        got = solver_state(solver, src, nvar)
        assert np.isfinite(U).all() and np.array_equal(got, U) and err == ref_err, (k, err, ref_err)
        out.append(np.append(got, err))
    return np.array(out)


def solver_form(solver):
    """[fused, steps, fused_steps] of ``tf_erk_info``: which form the solver's explicit steps took."""
    info = solver.erk_info()
    return np.array([info["fused"], info["steps"], info["fused_steps"]], dtype=float)


# --------------------------------------------------------------------------------------------------- order
ORDER_N, ORDER_T, ORDER_STEPS = 64, 0.4, (4, 8, 16, 32)
ORDER_P = {"SSPRK3": 3, "RK4": 4, "BS23": 3, "DOPRI5": 5}


def order_inputs():
    x = np.linspace(0.0, 1.0, ORDER_N, endpoint=False)
    return dict(x=x, U=np.cos(2 * np.pi * 5 * x)), dict(k=1e-3, c=0.03, periodic=True)


@lru_cache(maxsize=None)
def order_reference():
    """expm(T J) U0 with J the model's own dense Jacobian (constant: the model is linear)."""
    from scipy.linalg import expm
    from tests.parity_cases import oracle_model
    fd, pars = order_inputs()
    mo = oracle_model("M1_advdiff")
    J = np.asarray(mo.J(mo.fields_template(**fd), pars).todense())
    return expm(ORDER_T * J) @ fd["U"]


def check_order(backend, tab_name):
    """(5) M1_advdiff, periodic, N = 64 on [0, 1), T = 0.4 in 4, 8, 16 and 32 steps against the matrix
    exponential: each of the three observed orders log2(e_n / e_2n) is at least p - 0.1.  The yardstick
    alone gives 3.01-3.06 (SSPRK3, BS23; errors 3.8e-5 -> 6.9e-8), 4.01-4.06 (RK4; 1.0e-6 -> 2.3e-10) and
    5.03-5.12 (DOPRI5; 4.8e-9 -> 1.3e-13) on this input: above round-off throughout."""
    fd, pars = order_inputs()
    m = device_model("advdiff", backend)
    ref, errs = order_reference(), []
    for n in ORDER_STEPS:
        sch, f, t = general(m, tab_name), m.fields_template(**fd), 0.0
        for _ in range(n):
            t, f = sch(t, f, ORDER_T / n, pars)
        errs.append(np.abs(f.uflat - ref).max())
    orders = [np.log2(errs[i] / errs[i + 1]) for i in range(3)]
    print("%s: errors %s, observed orders %s" % (tab_name, ["%.3e" % e for e in errs], ["%.3f" % o for o in orders]))
    assert min(orders) >= ORDER_P[tab_name] - 0.1, (tab_name, errs, orders)
    return errs, orders


# ----------------------------------------------------------------------------------------------- controller
class NumpyERK(schemes.ERK_general):
    """The controller of ERK_general (inherited untouched) driven by the NumPy step: ``_fixed_step`` is the
    yardstick on host containers.  Null hook only (a landing step with a hook pokes a device slot)."""

    def __init__(self, case, fd, pars, tab_name, **kw):
        tab = ERK_TABLEAUX[tab_name]
        super().__init__(_symbolic_model(case)[0], tab.a, tab.b, b_err=tab.b_err, order=tab.order, **kw)
        self._F = numpy_F(case, fd, pars)
        self.log = []

    def _fixed_step(self, t, fields, dt, pars, hook=null_hook, hook_after=False, want_err=True, err_slot=None):
        assert hook is null_hook and err_slot is None
        new, err = numpy_step(self._F, fields.uflat, dt, self._a, self._b, self._d)
        out = fields.copy()
        out.fill(new)
        self.log.append((dt, err))
        return t + dt, out, err


def logged(scheme):
    """Record (dt, err) of every ``_fixed_step`` of a device scheme in ``scheme.log``."""
    inner, scheme.log = scheme._fixed_step, []

    def fixed_step(t, fields, dt, *a, **k):
        out = inner(t, fields, dt, *a, **k)
        scheme.log.append((dt, out[2]))
        return out
    scheme._fixed_step = fixed_step
    return scheme


def check_controller(backend, tab_name, N=203, ncalls=12, tol=1e-6, call_dt=0.05, start=None):
    """(6) ``ncalls`` calls of the adaptive scheme against the same controller driven by the NumPy step: the
    sequence of trial dts, the estimates (hence the accept / reject decisions), the returned t and the
    states, bit for bit.  ``start``: the controller's internal dt before the first call."""
    gc.collect()
    fd, pars, _ = inputs("advdiff", N, True)
    m = device_model("advdiff", backend)
    dev = logged(getattr(schemes, tab_name)(m, tol=tol))
    ref = NumpyERK("advdiff", fd, pars, tab_name, time_stepping=True, tol=tol)
    assert type(dev)._variable_step is schemes.ROW_general._variable_step is type(ref)._variable_step
    if start is not None:
        dev._internal_dt = ref._internal_dt = start
    fa, fb = m.fields_template(**fd), ref._model.fields_template(**fd)
    ta = tb = 0.0
    for k in range(ncalls):
        with np.errstate(all="ignore"):
            ta, fa = dev(ta, fa, call_dt, pars)
            tb, fb = ref(tb, fb, call_dt, pars)
        assert ta == tb, (tab_name, k)
        x, y = fa.copy().uflat, fb.uflat
        assert np.isfinite(y).all() and np.array_equal(x, y), (tab_name, "call %d" % k, np.abs(x - y).max())
        assert dev._internal_dt == ref._internal_dt and dev._err == ref._err, (tab_name, k)
    assert len(dev.log) == len(ref.log) and len(dev.log) >= ncalls
    assert np.array_equal(np.array(dev.log, dtype=float), np.array(ref.log, dtype=float)), tab_name
    rejected = sum(1 for _, err in dev.log if err is not None and err > tol)
    print("%s tol=%g: %d steps in %d calls, %d rejected" % (tab_name, tol, len(dev.log), ncalls, rejected))
    return dev.log, rejected


def check_controller_limits(backend, tab_name="BS23"):
    """(6) ``max_iter`` and ``dt_min`` raise RuntimeError, as for the Rosenbrock classes."""
    import pytest
    fd, pars, _ = inputs("advdiff", 203, True)
    m = device_model("advdiff", backend)
    with pytest.raises(RuntimeError, match="max iterations"):
        sch = getattr(schemes, tab_name)(m, tol=1e-10, max_iter=2)
        sch._internal_dt = 1e-4                      # the tolerance holds dt near 2e-3: 26 steps to t = 0.05
        sch(0.0, m.fields_template(**fd), 0.05, pars)
    with pytest.raises(RuntimeError, match="less than authorized"):
        sch = getattr(schemes, tab_name)(m, tol=1e-10, dt_min=1.0)
        sch._internal_dt = 1e-4
        sch(0.0, m.fields_template(**fd), 0.05, pars)


# ------------------------------------------------------------------------------------------- public drivers
def check_simulation_fixed(backend, with_probe):
    """(7) ``Simulation(..., scheme=schemes.RK4, time_stepping=False)``: the states of eight iterations
    equal the yardstick's; on the GPU with a probe attached, whose rows are the maxima of those states."""
    N, dt = 203, 1e-3
    fd, pars, _ = inputs("advdiff", N, True)
    m = device_model("advdiff", backend)
    sim = Simulation(m, dict(fd), dict(pars), dt, scheme=schemes.RK4, time_stepping=False)
    if with_probe:
        sim.add_probe("top", "U", reduce="max")
    ref, _ = numpy_run("advdiff", N, True, "RK4", nsteps=8, dt=dt)
    for k, (t, f) in zip(range(8), sim):
        assert np.array_equal(f.copy().uflat, ref[k]), k
    if with_probe:
        t, top = sim.probes["top"]
        assert np.array_equal(top[1:9].ravel(), np.array([r.max() for r in ref]))
    return sim


def check_simulation_step_doubling(backend):
    """(7) ``Simulation(..., scheme=schemes.SSPRK3)`` with the default step-doubling wrapper: it runs through
    the wrapper's step-by-step path (``_device_desc()`` is None), and the states equal the oracle's wrapper
    (the reference's logic, oracle/numpy_path.py) applied to the NumPy step."""
    N, dt = 203, 1e-2
    fd, pars, _ = inputs("advdiff", N, True)
    m = device_model("advdiff", backend)
    assert schemes.SSPRK3(m)._device_desc() is None
    sim = Simulation(m, dict(fd), dict(pars), dt, scheme=schemes.SSPRK3)
    mo = _symbolic_model("advdiff")[0]
    F, (tab, _) = numpy_F("advdiff", fd, pars), tableau("SSPRK3")

    def np_scheme(t, fields, h, p, hook=None):
        out = fields.copy()
        out.fill(numpy_step(F, fields.uflat, h, tab.a, tab.b)[0])
        return t + h, out
    wrapped = ora.time_stepping(np_scheme)
    fr, tr = mo.fields_template(**fd), 0.0
    for k, (t, f) in zip(range(4), sim):
        tr, fr = wrapped(tr, fr, dt, pars, None)
        assert t == tr and np.array_equal(f.copy().uflat, fr.uflat), (k, np.abs(f.copy().uflat - fr.uflat).max())


def check_ensemble(backend, scheme="RK4", N=203, steps=5, dt=1e-3):
    """(7) Three members of different parameters: member 1 equals a single-member ensemble with its
    parameters bit for bit, and the yardstick; no factorisation was made."""
    fd, pars, _ = inputs("advdiff", N, True)
    m = device_model("advdiff", backend)
    ks = np.array([1e-3, 2e-3, 5e-4])
    U = np.array([fd["U"], 0.5 * fd["U"] + 0.1, fd["U"][::-1].copy()])
    ens = Ensemble(m, fd["x"], dict(U=U), dict(k=ks, c=0.03), True, scheme=scheme)
    one = Ensemble(m, fd["x"], dict(U=U[1:2]), dict(k=ks[1:2], c=0.03), True, scheme=scheme)
    for _ in range(steps):
        ens.step(dt)
        one.step(dt)
    a, b = np.asarray(ens.state()), np.asarray(one.state())
    assert np.isfinite(a).all() and np.array_equal(a[:, 1, :], b[:, 0, :])
    assert not np.array_equal(a[:, 0, :], a[:, 1, :])
    tab, _ = tableau(scheme)
    Fn = numpy_F("advdiff", fd, dict(k=ks[1], c=0.03, periodic=True))
    ref = U[1].copy()
    for _ in range(steps):
        ref = numpy_step(Fn, ref, dt, tab.a, tab.b)[0]
    assert np.array_equal(a[0, 1, :], ref)
    assert ens.solver.counters()["factorisations"] == 0 and one.solver.counters()["factorisations"] == 0
    ens.close()
    one.close()


def check_no_factorisation(backend):
    """(7) ``tf_solver_counters`` after explicit steps on a fresh solver: no factorisation, no check."""
    solver, fd, pars, dt = raw_solver(backend, "film", 203, True)
    for tab_name in TABLEAUX:
        raw_steps(solver, 3, tab_name, (dt, dt))
    c = solver.counters()
    assert c["factorisations"] == 0 and c["checks"] == 0 and c["replans"] == 0, c


# ------------------------------------------------------------------------- fused against unfused: the dump
def dump_cases():
    for case in CASES:
        for N in SHAPES:
            for periodic in (True, False):
                yield case, N, periodic


def dump(path):
    """States (the last of five steps of every tableau; every step's for N = 203) and estimates of every
    case, the hook cases, the graph run and the NaN case -> ``path`` (npz)."""
    out = {}
    for case, N, periodic in dump_cases():
        for tab_name in TABLEAUX:
            states, errs = device_run(None, case, N, periodic, tab_name)
            key = "%s|%d|%d|%s" % (case, N, periodic, tab_name)
            out[key + "|U"] = np.array(states if N == 203 else states[-1:])
            if errs[0] is not None:
                out[key + "|err"] = np.array(errs, dtype=float)
    for which in HOOKS:
        for tab_name in TABLEAUX:
            states, errs = device_run(None, "advdiff", 203, False, tab_name, hook=HOOKS[which])
            out["hook|%s|%s|U" % (which, tab_name)] = np.array(states)
    states, errs = graph_run(None)
    out["graph|U"], out["graph|err"] = np.array(states), np.array(errs, dtype=float)
    for tab_name, (U, err) in check_nan_wins(None).items():
        out["nan|%s|U" % tab_name], out["nan|%s|err" % tab_name] = U, np.array([err])
    out["zero|U"] = check_zero_coefficient_rule(None)
    out["heun|U"] = check_window_term_outside_the_update(None)
    # which form the steps above took: the raw solver of the NaN / zero / graph cases, and a stepper's
    out["info|raw"] = solver_form(raw_solver(None, "advdiff", 203, True)[0])
    m, (fd, pars, dt) = device_model("film", None), inputs("film", 203, True)
    _, f, _ = general(m, "DOPRI5")._fixed_step(0.0, m.fields_template(**fd), dt, pars, hook_after=True)
    out["info|stepper"] = solver_form(f._device_backing().stepper.solver)
    np.savez(path, **out)


def dump_graph(path):
    """The graph run alone (started with ``TRIFLOW_GRAPHS=1`` and ``=0``)."""
    states, errs = graph_run(None)
    np.savez(path, **{"graph|U": np.array(states), "graph|err": np.array(errs, dtype=float)})


if __name__ == "__main__":
    {"dump": dump, "dump_graph": dump_graph}[sys.argv[1]](sys.argv[2])
