"""Expression hooks on the MI355X: ``tf_hook_apply`` against the hand-written Python functions of
tests/hook_cases.py, and runs with an ``ExpressionHook`` against the same runs with the hand-written callable as
``hook`` -- the generic path that brings the state to the host -- state by state, bit for bit: a program
applied one time too few or too many, or at the wrong ``t``, changes the bits."""
import numpy as np
import pytest

from tests import hook_cases as hc
from triflow_amd import Simulation, schemes
from triflow_amd._capi import DeviceSolver
from triflow_amd.device import DirichletHook, ExpressionHook, Stepper, null_hook, stepper_for
from triflow_amd.ensemble import Ensemble

pytestmark = pytest.mark.gpu

T = 0.37
GRIDS = (203, 4099)
STEPS = 5


def bits(a):
    return np.asarray(a, dtype=float).tobytes()


def snapshot(model, fields):
    return {n: np.array(fields[n], dtype=float) for n in model._dep_vars}


def assert_same_states(a, b, what):
    assert len(a) == len(b)
    for k, (sa, sb) in enumerate(zip(a, b)):
        for n in sa:
            assert bits(sa[n]) == bits(sb[n]), "%s: step %d, %s differs at %s" % (
                what, k, n, np.flatnonzero(sa[n].view(np.uint64) != sb[n].view(np.uint64))[:8])


def fresh_solvers(model):
    """The next run on ``model`` gets solvers of its own.  What a solver has learnt about its factorisations
    (the verdicts of the accuracy guard: which solves are checked, how many refinement sweeps they take)
    stays with it from run to run, and two runs are compared here step by step, to the bit: each starts from
    a solver that has seen nothing."""
    compiled = model._device
    compiled.__dict__.pop("_steppers", None)
    compiled.release()


def pin_guard(model, fields, pars):
    """The stepper the next run on ``model`` takes, with the banded solver's accuracy guard switched off
    (``refine=0``: plain elimination, no check, no monitor, no refinement sweep).  The guard decides by what the
    host has seen: a synchronising call (``tf_get_state``, ``tf_set_state``: ``tf_solver::check_status``) looks at
    the monitor's worst backward error, and a value above the trigger makes the next factorisation a checked and
    refined one.  The generic path of a Python hook synchronises in every scheme call, the resident path of a
    program never does inside a ``Simulation`` step, so over the many factorisations of the step-doubling
    trials the two check and refine different solves (measured, ROS2, N = 4099, default solver: after two
    ``Simulation`` steps both runs had made 408 factorisations, the callable's run 104 checks, the program's
    95), which moves last bits at a few nodes -- with the same hook applications at the same times.  The
    comparison is about those, so both runs get the same, fixed solver."""
    compiled = model._device
    periodic = bool(pars["periodic"])
    mask = compiled.parvec_mask_of([pars[k] for k in compiled.pars])
    stepper = Stepper(compiled, fields.size, periodic, mask, refine=0)
    compiled.__dict__.setdefault("_steppers", {})[(fields.size, periodic, mask, ())] = stepper
    return stepper


def film_inputs(N, fresh=True):
    model = hc.model("film", compiled=True)
    if fresh:
        fresh_solvers(model)
    x = np.linspace(0.0, 10.0, N)
    h = 1 + 0.1 * np.cos(2 * np.pi * 2 * x / 10)
    fields = model.fields_template(x=x, h=h, q=0.5 * h * h, T=np.sin(2 * np.pi * x / 10))
    return model, fields, dict(hc.pars_of("film", N), periodic=False)


def as_callable(reference):
    """The hand-written function as a hook of the reference's protocol."""
    def hook(t, fields, pars):
        reference(t, fields, pars)
        return fields, pars
    return hook


# ---- one application ------------------------------------------------------------------------------
@pytest.mark.parametrize("N", GRIDS)
@pytest.mark.parametrize("name", sorted(hc.CASES))
def test_apply_equals_hand_written(name, N):
    mname, statements, _ = hc.case(name, N)
    model = hc.model(mname, compiled=True)
    hook = ExpressionHook(model, statements)
    pars = dict(hc.pars_of(mname, N), periodic=False)
    for special in (False, True):
        before, want = hc.expected(name, N, T, special=special)
        fields = model.fields_template(**before)
        out = stepper_for(model, fields, pars).apply_hook(hook, T, fields, pars)
        assert out._device_backing() is not None
        for n in model._dep_vars:
            assert bits(out[n]) == bits(want[n]), (name, N, special, n)
        for n in model._dep_vars:                    # the input container is what it was
            assert bits(fields[n]) == bits(before[n])


# ---- stepping: the generic path of the hand-written callable is the yardstick -----------------------
def explicit_dt(N):
    dx = 10.0 / (N - 1)
    return 0.02 * dx ** 4 / 0.01          # (We * dxxxxh sets the explicit limit)


SCHEMES = {
    "theta1": (lambda m: schemes.Theta(m, theta=1), dict(scheme=schemes.Theta, theta=1), 1e-3),
    "theta05": (lambda m: schemes.Theta(m, theta=0.5), dict(scheme=schemes.Theta, theta=0.5), 1e-3),
    "ros2": (schemes.ROS2, dict(scheme=schemes.ROS2), 1e-3),
    "rodaspr": (lambda m: schemes.RODASPR(m, time_stepping=True), dict(scheme=schemes.RODASPR), 1e-3),
    "ssprk3": (schemes.SSPRK3, dict(scheme=schemes.SSPRK3), None),
    "dopri5": (lambda m: schemes.DOPRI5(m, time_stepping=True), dict(scheme=schemes.DOPRI5), None),
}


def run_scheme(make, N, hook, dt):
    model, fields, pars = film_inputs(N)
    scheme, t, states = make(model), 0.0, []
    for _ in range(STEPS):
        t, fields = scheme(t, fields, dt, pars, hook=hook)
        states.append(snapshot(model, fields))
    return states


def run_simulation(kw, N, hook, dt, wrapper):
    model, fields, pars = film_inputs(N)
    # (the wrapper's error is a norm of the difference of two states: the maximum norm, which does not depend
    # on the order of the nodes -- the generic path takes it with NumPy, the device path with a reduction)
    extra = dict(ord=np.inf) if wrapper else {}
    if wrapper:
        pinned = pin_guard(model, fields, pars)
        assert stepper_for(model, fields, pars) is pinned
    # (time_stepping also reaches the constructors of RODASPR and DOPRI5: their own control is on inside the
    # wrapper and off without it -- the fixed-step forms of the two tableaux)
    sim = Simulation(model, fields, pars, dt, hook=hook, time_stepping=wrapper, **kw, **extra)
    states = []
    for _ in range(STEPS):
        next(sim)
        states.append(snapshot(model, sim.fields))
    if wrapper:                                      # the run was on the pinned solver, and nothing was checked
        assert stepper_for(model, sim.fields, pars) is pinned and pinned.solver.counters()["checks"] == 0
    return states


@pytest.mark.parametrize("N", GRIDS)
@pytest.mark.parametrize("name", sorted(SCHEMES))
def test_scheme_objects_equal_the_callable(name, N):
    make, _, dt = SCHEMES[name]
    dt = dt or explicit_dt(N)
    model = hc.model("film", compiled=True)
    _, statements, reference = hc.case("film_full", N)
    want = run_scheme(make, N, as_callable(reference), dt)
    got = run_scheme(make, N, ExpressionHook(model, statements), dt)
    assert np.isfinite(want[-1]["h"]).all()
    assert_same_states(got, want, "%s N=%d" % (name, N))


@pytest.mark.parametrize("wrapper", [False, True])
@pytest.mark.parametrize("N", GRIDS)
@pytest.mark.parametrize("name", sorted(SCHEMES))
def test_simulation_equals_the_callable(name, N, wrapper):
    """Without the wrapper a step is one factorisation and the default solver serves both runs.  Inside the
    wrapper both runs take a solver whose accuracy guard is off (``pin_guard``: with the default one,
    ros2-4099-True differed in the last bit of ``q`` at 8 of 4099 nodes, none of them assigned by the
    program, from step 1 on)."""
    _, kw, dt = SCHEMES[name]
    dt = dt or explicit_dt(N)
    model = hc.model("film", compiled=True)
    _, statements, reference = hc.case("film_full", N)
    want = run_simulation(kw, N, as_callable(reference), dt, wrapper)
    got = run_simulation(kw, N, ExpressionHook(model, statements), dt, wrapper)
    assert np.isfinite(want[-1]["h"]).all()
    assert_same_states(got, want, "%s N=%d wrapper=%s" % (name, N, wrapper))


# ---- replay ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("make", [schemes.ROS2, lambda m: schemes.Theta(m, theta=1), schemes.SSPRK3],
                         ids=["ros2", "theta", "ssprk3"])
def test_replayed_steps_see_their_own_t(make):
    """N = 203: fixed steps are replayed from a captured graph from the third one on; the inlet node of
    every step holds the value of that step's own t."""
    N, dt = 203, 1e-3
    model, fields, pars = film_inputs(N)
    if make is schemes.SSPRK3:
        dt = explicit_dt(N)
    _, statements, reference = hc.case("film_inlet", N)
    hook = ExpressionHook(model, statements)
    assert hook.idempotent and hook.time_dependent
    scheme, t, inlet, states = make(model), 0.0, [], []
    for _ in range(6):
        t, fields = scheme(t, fields, dt, pars, hook=hook)
        inlet.append((t, float(np.asarray(fields["h"])[0])))
        states.append(snapshot(model, fields))
    for t_n, value in inlet:
        assert value == 1 + pars["eps"] * np.sin(2 * np.pi * pars["c"] * t_n), (t_n, value)
    assert len({v for _, v in inlet}) == 6
    want = run_with(make, N, as_callable(reference), dt, 6)
    assert_same_states(states, want, "replay")


def run_with(make, N, hook, dt, steps, fresh=True):
    model, fields, pars = film_inputs(N, fresh)
    scheme, t, states = make(model), 0.0, []
    for _ in range(steps):
        t, fields = scheme(t, fields, dt, pars, hook=hook)
        states.append(snapshot(model, fields))
    return states


# ---- BDF2 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["film_open", "film_inlet"])
def test_bdf2(case, monkeypatch):
    """The sponge program is not idempotent: BDF2 uses it as the callable it is (the documented fallback);
    the inlet program runs on the device.  Both equal the hand-written callable."""
    N, dt = 203, 1e-3
    model = hc.model("film", compiled=True)
    _, statements, reference = hc.case(case, N)
    hook = ExpressionHook(model, statements)
    want = run_with(schemes.BDF2, N, as_callable(reference), dt, STEPS)
    downloads = []
    orig = DeviceSolver.get_state
    monkeypatch.setattr(DeviceSolver, "get_state", lambda self, *a, **k: downloads.append(1) or orig(self, *a, **k))
    model_, fields, pars = film_inputs(N)
    scheme, t, got = schemes.BDF2(model_), 0.0, []
    for _ in range(STEPS):
        t, fields = scheme(t, fields, dt, pars, hook=hook)
        got.append(fields)
    on_device = not downloads
    got = [snapshot(model, f) for f in got]
    assert on_device == hook.idempotent
    assert_same_states(got, want, "BDF2 " + case)


# ---- residency -------------------------------------------------------------------------------------
def test_state_stays_resident(monkeypatch):
    calls = dict(up=0, down=0)
    for meth, key in (("set_state", "up"), ("get_state", "down"), ("get_state_flat", "down")):
        orig = getattr(DeviceSolver, meth)

        def counted(self, *a, _orig=orig, _key=key, **k):
            calls[_key] += 1
            return _orig(self, *a, **k)
        monkeypatch.setattr(DeviceSolver, meth, counted)
    N = 4099
    model, fields, pars = film_inputs(N)
    hook = ExpressionHook(model, hc.case("film_full", N)[1])
    sim = Simulation(model, fields, pars, 1e-3, hook=hook, scheme=schemes.ROS2, time_stepping=False)
    for _ in range(20):
        t, f = next(sim)
        assert f._device_backing() is not None and f._device_backing().valid()
    assert calls == dict(up=1, down=0), calls
    assert np.isfinite(np.asarray(sim.fields["h"])).all()
    assert calls["down"] == 1


# ---- ensemble --------------------------------------------------------------------------------------
def test_ensemble_members_get_their_own_parameters():
    N, nsys = 203, 3
    model = hc.model("film", compiled=True)
    _, statements, reference = hc.case("film_full", N)
    members = [hc.fields_of("film", N, seed=e) for e in range(nsys)]
    eps = np.array([0.25, 0.5, 0.125])
    base = hc.pars_of("film", N)
    ens = Ensemble(model, members[0]["x"], {n: np.array([m[n] for m in members]) for n in ("h", "q", "T")},
                   dict(base, eps=eps), periodic=False, hook=ExpressionHook(model, statements))
    try:
        ens.t = T
        before = ens.state()
        ens.apply_hook()
        after = ens.state()
        for e in range(nsys):
            f = {"x": members[e]["x"], **{n: before[k, e].copy() for k, n in enumerate(("h", "q", "T"))}}
            reference(T, f, dict(base, eps=eps[e]))
            for k, n in enumerate(("h", "q", "T")):
                assert bits(after[k, e]) == bits(f[n]), (e, n)
        assert len({float(after[0, e, 0]) for e in range(nsys)}) == nsys
        ens.step(1e-3)                               # the step functions run it too, per member
        ens.sync()
        stepped = ens.state()
        for e in range(nsys):
            assert stepped[0, e, 0] == 1 + eps[e] * np.sin(2 * np.pi * base["c"] * (T + 1e-3))
    finally:
        ens.close()


# ---- what exists goes the way it went ----------------------------------------------------------------
def test_dirichlet_and_null_hook_unchanged_by_an_attached_program():
    N, dt = 203, 1e-3
    model = hc.model("film", compiled=True)
    dirichlet = DirichletHook(h={0: 1.0, -1: 1.0}, q={0: lambda t: 0.5 + t})

    def attach_and_detach():
        """A step with a program and one without on the stepper the next run uses."""
        _, fields, pars = film_inputs(N)
        stepper = stepper_for(model, fields, pars)
        program = ExpressionHook(model, hc.case("film_full", N)[1])
        schemes.ROS2(model)(0.0, fields, dt, pars, hook=program)
        assert stepper._attached is not None
        schemes.ROS2(model)(0.0, fields, dt, pars, hook=null_hook)
        assert stepper._attached is None             # detached: nothing is left behind
        return stepper

    def runs(attached):
        out = {}
        for hname, hook in (("dirichlet", dirichlet), ("null", null_hook)):
            for sname, make in (("ros2", schemes.ROS2), ("theta", lambda m: schemes.Theta(m, theta=1)),
                                ("ssprk3", schemes.SSPRK3)):
                fresh_solvers(model)
                stepper = attach_and_detach() if attached else None
                out[hname, sname] = run_with(make, N, hook, explicit_dt(N) if sname == "ssprk3" else dt, 4,
                                             fresh=False)
                if attached:
                    _, fields, pars = film_inputs(N, fresh=False)
                    assert stepper_for(model, fields, pars) is stepper      # the run was on that stepper
        return out
    before = runs(False)                             # before any ExpressionHook exists
    after = runs(True)
    for key in before:
        assert_same_states(after[key], before[key], "%s / %s after a program was attached" % key)
