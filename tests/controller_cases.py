"""Checks of the adaptive Rosenbrock controller (schemes.ROW_general._variable_step / _trial) with the first
trial of the next call queued ahead (QUEUE_NEXT_TRIAL), shared by the CPU suite (tests/test_controller.py, the
emulation) and the GPU suite (tests/test_gpu_controller.py, the HIP path).  The pieces below the controller --
tf_step_row_queued + tf_read_err give the bits of tf_step_row's estimate -- are held in tests/reduction_cases.py;
here the controller built on them is run through the branch that takes a queued step, against the controller that
launches every trial when it needs it (bit for bit) and against the oracle's literal sequence.

Two helpers carry every case:

* :func:`snapshot` reads a state without detaching the container from its device slot (``f.copy().uflat``;
  ``f.uflat`` would materialise ``f``, and a host container never takes a queued step);
* :class:`Tally` counts, per call of the scheme, the trials, which of them the scheme launched itself and which
  it took from the queue.  It looks at what ``_trial`` launches, not at the condition by which it decides.
"""
import contextlib
import gc
from functools import lru_cache

import numpy as np

from oracle import corpus, numpy_path as ora
from triflow_amd import Simulation, schemes
from triflow_amd.device import DirichletHook

from tests.parity_cases import device_model as _new_device_model, oracle_model

NCALLS = 22
T0 = 0.3
ROW = schemes.ROW_general


@lru_cache(maxsize=None)
def device_model(name, backend):
    """One model, hence one stepper per grid, for all runs of a case: a run starts on the solver, the
    state slots and the mailboxes the run before it left behind."""
    return _new_device_model(name, backend)


def snapshot(f):
    """The state of ``f`` as a flat host array; ``f`` stays attached to its device slot."""
    u = f.copy().uflat
    backing = f._device_backing()
    assert backing is not None and backing.valid(), "the snapshot detached the container"
    return u


class Tally:
    """What the adaptive schemes did while :func:`tally` was active.  ``calls[id(scheme)]`` is a list with one
    entry per ``_variable_step``: the list of its trials, each ``dict(own, spec, err, rejected)``.  ``own``: the
    trial launched a step from the very container it was asked to advance; a trial that did not took the
    step an earlier call had queued.  ``spec``: it queued a step from another container behind it."""

    def __init__(self):
        self.calls = {}

    def of(self, scheme):
        return self.calls.get(id(scheme), [])

    def hits(self, scheme):
        """Per call: trials minus the trials the scheme launched itself."""
        return [sum(1 for tr in call if not tr["own"]) for call in self.of(scheme)]

    def trials(self, scheme):
        """Per call: the accept (False) / reject (True) flags of its trials, in order."""
        return [tuple(tr["rejected"] for tr in call) for call in self.of(scheme)]

    def rejected_with_speculation(self, scheme):
        return sum(1 for call in self.of(scheme) for tr in call if tr["rejected"] and tr["spec"])


@contextlib.contextmanager
def tally():
    """Wrap ``ROW_general._variable_step`` / ``_trial`` / ``_fixed_step`` for the duration of a case."""
    rec = Tally()
    orig_v, orig_t, orig_f = ROW._variable_step, ROW._trial, ROW._fixed_step
    current = {}                                    # id(scheme) -> the trial being made

    def variable_step(self, *a, **k):
        rec.calls.setdefault(id(self), []).append([])
        return orig_v(self, *a, **k)

    def trial(self, t, fields, *a, **k):
        entry = dict(own=False, spec=False, queued=0, fields=fields)
        current[id(self)] = entry
        try:
            out = orig_t(self, t, fields, *a, **k)
        finally:
            current.pop(id(self), None)
        err = out[2]
        rec.calls[id(self)][-1].append(dict(own=entry["own"], spec=entry["spec"], queued=entry["queued"],
                                            err=err, rejected=bool(err > self._tol)))
        return out

    def fixed_step(self, t, fields, *a, **k):
        entry = current.get(id(self))
        if entry is not None:                         # (else: a landing step, outside every trial)
            if k.get("err_slot") is not None:
                entry["queued"] += 1
            if fields is entry["fields"]:
                entry["own"] = True
            else:
                entry["spec"] = True
        return orig_f(self, t, fields, *a, **k)

    ROW._variable_step, ROW._trial, ROW._fixed_step = variable_step, trial, fixed_step
    try:
        yield rec
    finally:
        ROW._variable_step, ROW._trial, ROW._fixed_step = orig_v, orig_t, orig_f


class Run:
    """One driven sequence: per call the state, the returned t, the scheme's _err and _internal_dt."""

    def __init__(self):
        self.states, self.t, self.err, self.idt = [], [], [], []
        self.hits, self.trials, self.rejected_with_speculation = [], [], 0

    def record(self, scheme, t, f):
        self.states.append(snapshot(f))
        self.t.append(t)
        self.err.append(scheme._err)
        self.idt.append(scheme._internal_dt)


def assert_same_run(a, b, what):
    """Bit for bit: states, returned t, error estimates and the controller's step, call by call."""
    assert len(a.states) == len(b.states)
    for k, (x, y) in enumerate(zip(a.states, b.states)):
        assert np.isfinite(x).all(), (what, k)
        assert np.array_equal(x, y), (what, "state of call %d" % k, np.abs(x - y).max())
    assert np.array_equal(np.array(a.t), np.array(b.t)), (what, "t")
    assert np.array_equal(np.array(a.err, dtype=float), np.array(b.err, dtype=float)), (what, "_err")
    assert np.array_equal(np.array(a.idt, dtype=float), np.array(b.idt, dtype=float)), (what, "_internal_dt")


def drive(backend, cfg, N, make, queue=True, reuse=True, before=None, ncalls=NCALLS, scale=None):
    """``ncalls`` calls of ``make(model)`` on BASELINE configuration ``cfg`` from t = 0.3.  ``before(k, ctx)``
    runs before call ``k`` and may change ``ctx["f"]``, ``ctx["p"]`` (the parameter dict handed in: one object,
    call after call) and ``ctx["dt"]``.  ``scale(fd)`` edits the initial fields."""
    gc.collect()          # containers of earlier runs that nobody has collected yet would still hold state slots
    name, fd, pars, dt, _ = corpus.config_inputs(cfg, N)
    if scale is not None:
        fd = scale(dict(fd))
    m = device_model(name, backend)
    scheme = make(m)
    scheme.QUEUE_NEXT_TRIAL, scheme.REUSE_TRIAL_AS_LANDING = queue, reuse
    ctx = dict(f=m.fields_template(**fd), p=dict(pars), dt=dt, t=T0, scheme=scheme, model=m)
    run = Run()
    with tally() as rec, np.errstate(all="ignore"):
        for k in range(ncalls):
            if before is not None:
                before(k, ctx)
            ctx["t"], ctx["f"] = scheme(ctx["t"], ctx["f"], ctx["dt"], ctx["p"])
            run.record(scheme, ctx["t"], ctx["f"])
    run.hits, run.trials = rec.hits(scheme), rec.trials(scheme)
    run.rejected_with_speculation = rec.rejected_with_speculation(scheme)
    run.solver = ctx["f"]._device_backing().stepper.solver
    return run


def on_and_off(backend, cfg, N, make, **kw):
    """The same sequence with the queue on and off; the off run took nothing from a queue."""
    on = drive(backend, cfg, N, make, queue=True, **kw)
    off = drive(backend, cfg, N, make, queue=False, **kw)
    assert sum(off.hits) == 0, off.hits
    return on, off


# ------------------------------------------------------------------------------------------------- the cases
#: (scheme, tol) pairs of the film model (config 3, 400 nodes, dt = 1e-3) at which the plain controller settles
#: on the caller's dt, so that a queued step can be the one asked for -> steps taken from the queue in 22 calls on
#: the emulation.  (At tol = 1e-5 all three schemes keep their own step below dt, 18 trials per call: no call can
#: take a queued step, and none does.)
HIT_PAIRS = {("RODASPR", 1e-1): 20, ("RODASPR", 1e-3): 20, ("ROS3PRL", 1e-1): 20, ("ROS3PRL", 1e-3): 20,
             ("ROS3PRw", 1e-1): 20, ("ROS3PRw", 1e-3): 20}


#: steps taken from the queue, scheme calls in 13 iterations of ``Simulation`` with its defaults (emulation and
#: MI355X): the plain path does take queued steps -- the null hook hands the caller's parameter dict through
#: unchanged, and the ten fine steps of a step-doubling trial and the landing steps ask for the step the one
#: before queued.  A coarse step (10 dt' from the container the fine steps start from), the first call after the
#: parameter change and every call with a hook launch their own.
SIMULATION_HITS = {"plain": (17, 23), "pars": (16, 23), "hook": (0, 24)}


def _make(name, tol):
    return lambda m: getattr(schemes, name)(m, tol=tol)


def check_hit_branch_equals_plain(backend, name, tol):
    """(a) The branch of ``_trial`` that takes a queued step runs, and gives the bits of the controller that
    launches every trial when it needs it: states, returned t, ``_err`` and ``_internal_dt`` of 22 calls.
    Steps taken from the queue, of 22 calls: 20 for every pair of HIT_PAIRS on the emulation (the first call
    makes three or four trials of its own, the second is the first whose trial was queued by the one before)
    and on the MI355X; 0 with the queue off."""
    on, off = on_and_off(backend, 3, 400, _make(name, tol))
    print("%s tol=%g: steps taken from the queue per call %s" % (name, tol, on.hits))
    assert sum(on.hits) >= (15 if (name, tol) == ("RODASPR", 1e-1) else NCALLS // 2 + 1), on.hits
    assert max(on.hits) == 1                          # one per call: the call's first trial
    assert_same_run(on, off, (name, tol))
    return on


def _oracle_run(name, tol, cfg, N):
    mname, fd, pars, dt, _ = corpus.config_inputs(cfg, N)
    mo = oracle_model(mname)
    scheme = getattr(ora, name)(mo, tol=tol)
    inner, errs = scheme._fixed_step, []

    def fixed_step(*a, **k):
        out = inner(*a, **k)
        errs.append(out[2])
        return out
    scheme._fixed_step = fixed_step
    f, t, states, trials = mo.fields_template(**fd), T0, [], []
    with np.errstate(all="ignore"):
        for _ in range(NCALLS):
            del errs[:]
            t, f = scheme(t, f, dt, dict(pars))
            states.append(f.uflat.copy())
            trials.append(tuple(bool(e > tol) for e in errs[:-1]))        # the last step is the landing step
    return states, trials


def _rel_max(states, ref):
    return max(np.abs(a - b).max() / np.abs(b).max() for a, b in zip(states, ref))


EPS = np.finfo(float).eps


def check_hit_branch_against_oracle(backend, name, tol=1e-1):
    """(b) The default switches (queue and landing reuse on) against the oracle's adaptive scheme of the same
    name taken literally, landing step included: 22 calls on the film model.  The controller the suite already
    trusts -- both switches off, the literal sequence -- is measured against the oracle in the same test and has
    to be within the film model's step tolerance (parity_cases.STEP_TOL, 2e-7: two different solvers at cond
    ~ 1e10); the default run gets ten times the literal run's figure, floored at 100 eps (landing reuse moves a
    state by ~1e-16 relative per call, 22 calls, through that solver).  The accept / reject sequence of the
    trials of every call equals the oracle's in both runs.

    Relative max difference of the states, literal | default, on the MI355X and on the emulation alike
    (profiles/r14_queued_controller.txt): RODASPR 8.341e-17 | 8.341e-17, ROS3PRL 1.668e-16 | 1.668e-16, ROS3PRw
    1.668e-16 | 1.668e-16; 20 of the 22 default calls take a queued step.  The bound is therefore its floor,
    100 eps = 2.2e-14."""
    ref, ref_trials = _oracle_run(name, tol, 3, 400)
    literal = drive(backend, 3, 400, _make(name, tol), queue=False, reuse=False)
    default = drive(backend, 3, 400, _make(name, tol))
    e_lit, e_def = _rel_max(literal.states, ref), _rel_max(default.states, ref)
    print("%s tol=%g against the oracle: literal %.3e, default switches %.3e (%d steps from the queue)"
          % (name, tol, e_lit, e_def, sum(default.hits)))
    assert sum(literal.hits) == 0 and sum(default.hits) > NCALLS // 2, default.hits
    assert e_lit <= 2e-7, e_lit
    assert e_def <= max(10 * e_lit, 100 * EPS), (e_def, e_lit)
    assert literal.trials == ref_trials, (literal.trials, ref_trials)
    assert default.trials == ref_trials, (default.trials, ref_trials)
    return e_lit, e_def


def _set_par(key, value, at=12):
    def before(k, ctx):
        if k == at:
            ctx["p"][key] = value                     # the dict the scheme has been handed all along
    return before


def check_parameter_changed_in_place(backend, key, value):
    """(c) The caller changes a value of the parameter dict it hands in, between two calls: the step queued
    with the old value is not the step asked for."""
    make = _make("RODASPR", 1e-1)
    on, off = on_and_off(backend, 3, 400, make, before=_set_par(key, value))
    plain = drive(backend, 3, 400, make, queue=False)
    assert_same_run(on, off, ("in place", key))
    assert on.hits[12] == 0 and sum(on.hits) >= 15, on.hits
    assert not np.array_equal(off.states[12], plain.states[12])          # the change shows in the state
    assert np.array_equal(off.states[11], plain.states[11])


def _write_node(var, node, value, at=12):
    def before(k, ctx):
        if k == at:
            getattr(ctx["f"], var)[node] = value      # a point write queued on the device-backed container
            assert ctx["f"]._device_backing() is not None
    return before


def check_node_written_between_calls(backend, var, node, value):
    """(d) ``fields.h[0] = 1.05`` between two calls reaches the device: the step queued from the state
    before the write is not the step asked for."""
    make = _make("RODASPR", 1e-1)
    on, off = on_and_off(backend, 3, 400, make, before=_write_node(var, node, value))
    plain = drive(backend, 3, 400, make, queue=False)
    assert_same_run(on, off, ("write", var, node))
    assert on.hits[12] == 0 and sum(on.hits) >= 15, on.hits
    assert not np.array_equal(on.states[12], plain.states[12])           # the write arrived
    assert np.array_equal(on.states[11], plain.states[11])


def _simulation_run(backend, cfg, N, queue, hook=None, change=None, iters=13):
    gc.collect()
    name, fd, pars, dt, _ = corpus.config_inputs(cfg, N)
    m = device_model(name, backend)
    kw = {} if hook is None else {"hook": hook}
    sim = Simulation(m, dict(fd), dict(pars), dt, **kw)
    scheme = sim._scheme.__wrapped__                  # the RODASPR instance inside the step-doubling wrapper
    assert isinstance(scheme, schemes.RODASPR)
    scheme.QUEUE_NEXT_TRIAL = queue
    run = Run()
    with tally() as rec, np.errstate(all="ignore"):
        for k, (t, f) in zip(range(iters), sim):
            run.record(scheme, t, f)
            if change is not None and k == 6:
                change(sim)
    run.hits, run.trials = rec.hits(scheme), rec.trials(scheme)
    return run


def check_through_simulation(backend, variant):
    """(e) ``Simulation(model, fields, pars, dt)`` with its defaults -- adaptive RODASPR inside the step-doubling
    wrapper -- iterated 13 times: the queue on against off, bit for bit.  ``plain``; ``pars``: the caller sets
    ``simul.parameters["We"]`` after iteration 6; ``hook``: config 1 with its declarative Dirichlet hook -- a hook
    never rides the queue, no step is taken from it.

    Steps taken from the queue by the plain Simulation path: see SIMULATION_HITS (the wrapper alternates a
    coarse step of 10 dt' with ten fine steps of dt' from the same container object and parameter dict)."""
    if variant == "hook":
        args = dict(cfg=1, N=200, hook=DirichletHook(U={0: 1.0, -1: 0.0}))
    elif variant == "pars":
        args = dict(cfg=3, N=400, change=lambda sim: sim.parameters.__setitem__("We", 0.02))
    else:
        args = dict(cfg=3, N=400)
    on, off = _simulation_run(backend, queue=True, **args), _simulation_run(backend, queue=False, **args)
    print("Simulation [%s]: %d scheme calls, %d steps taken from the queue"
          % (variant, len(on.hits), sum(on.hits)))
    assert sum(off.hits) == 0
    if variant == "hook":
        assert sum(on.hits) == 0, on.hits
    assert_same_run(on, off, ("Simulation", variant))
    if variant == "pars":
        unchanged = _simulation_run(backend, queue=False, cfg=3, N=400)
        assert np.array_equal(on.states[6], unchanged.states[6])
        assert not np.array_equal(on.states[7], unchanged.states[7])
    return sum(on.hits), len(on.hits)


def _amplitude(a):
    def scale(fd):
        h = 1 + a * np.cos(2 * np.pi * 4 * fd["x"] / 100)
        fd["h"], fd["q"] = h, h ** 3
        return fd
    return scale


def _two_schemes(backend, queue, write):
    gc.collect()
    name, fd, pars, dt, _ = corpus.config_inputs(3, 400)
    dts = [dt, dt / 1000]
    m = device_model(name, backend)
    fds = [dict(fd), _amplitude(0.3)(dict(fd))]
    ss = [schemes.RODASPR(m, tol=1e-1), schemes.RODASPR(m, tol=1e-6)]
    fs, ts, ps, runs = [m.fields_template(**d) for d in fds], [T0, T0], [dict(pars), dict(pars)], [Run(), Run()]
    with tally() as rec, np.errstate(all="ignore"):
        for s in ss:
            s.QUEUE_NEXT_TRIAL = queue
        for k in range(NCALLS):
            if write and k == 12:
                fs[1].T[0] = 0.5
            for i in (0, 1):
                ts[i], fs[i] = ss[i](ts[i], fs[i], dts[i], ps[i])
                runs[i].record(ss[i], ts[i], fs[i])
    assert fs[0]._device_backing().stepper is fs[1]._device_backing().stepper      # one solver, one set of mailboxes
    for s, run in zip(ss, runs):
        run.hits, run.trials = rec.hits(s), rec.trials(s)
    return runs


def check_two_schemes_on_one_stepper(backend, write):
    """(f) Two RODASPR instances on one model and grid -- one solver, into whose estimate mailboxes both post --
    called alternately: amplitude 0.1, tol 1e-1, dt = 1e-3 and amplitude 0.3, tol 1e-6, dt = 1e-6.  Both settle on
    their caller's dt and take queued steps (20 of 22 each on the emulation); the estimates are ~1.4e-4 and
    ~2.6e-7.  (The estimate at the caller's dt is set by that dt, not by the tolerance: a tolerance alone that
    separated the estimates by orders of magnitude would keep the second scheme's own step below dt and so off
    the queue altogether.)  Queue on against off, bit for bit, states and above all ``_err`` / ``_internal_dt``:
    a scheme that read the other's estimate shows there first.  ``write``: the second scheme's container gets
    ``T[0] = 0.5`` before call 12 and then rejects trials (a condition of the case; 12 trials in that call)."""
    on, off = _two_schemes(backend, True, write), _two_schemes(backend, False, write)
    print("two schemes%s: steps taken from the queue %s" % (" + write" if write else "", [sum(r.hits) for r in on]))
    for i in (0, 1):
        assert sum(off[i].hits) == 0
        assert_same_run(on[i], off[i], ("two schemes", i))
    ratio = np.array(off[0].err, dtype=float)[2:] / np.array(off[1].err, dtype=float)[2:]
    assert (ratio > 30).all(), ratio                  # estimates that cannot be mistaken for each other
    assert min(sum(r.hits) for r in on) >= 10, [r.hits for r in on]
    if write:
        assert sum(map(sum, off[1].trials)) >= 1, off[1].trials
        assert on[1].hits[12] == 0
    else:
        assert min(sum(r.hits) for r in on) >= 15, [r.hits for r in on]
    return on


def check_rejected_trial_with_speculation(backend):
    """(g) A trial that had the next call's trial queued behind it is rejected: RODASPR at tol 1e-3, ``h[0] =
    1.3`` before call 12 (the trial of that call, at the caller's dt, lands on the target, so the next one is
    queued; its estimate then exceeds the tolerance).  That this happened is asserted.  Queue on against off:
    equal runs; neither raises at the next ``sync()``; the monitor's worst backward error is on the same side
    of the solver's refinement trigger (1e-11) in both, and neither went to the rescue plan.  (The monitor values
    themselves are not compared bit for bit: the sampled monitor looks at another node with every step
    launched, dropped ones included.)  Each run has a solver of its own."""
    make, before = _make("RODASPR", 1e-3), _write_node("h", 0, 1.3)
    out = []
    for queue in (True, False):
        device_model.cache_clear()                    # a fresh solver: its monitor and counters are this run's
        run = drive(backend, 3, 400, make, queue=queue, before=before)
        worst = run.solver.monitor_error()            # (before the synchronising call, which starts it afresh)
        run.solver.sync()                             # raises what the steps left
        out.append((run, worst, run.solver.counters()["replans"]))
    device_model.cache_clear()
    (on, mon_on, re_on), (off, mon_off, re_off) = out
    print("rejected with a step queued behind: %d; monitor %.3e | %.3e" % (on.rejected_with_speculation, mon_on, mon_off))
    assert on.rejected_with_speculation >= 1, on.trials
    assert sum(off.hits) == 0 and sum(on.hits) > 0
    assert_same_run(on, off, "rejected trial")
    assert np.isfinite([mon_on, mon_off]).all() and (mon_on <= 1e-11) == (mon_off <= 1e-11), (mon_on, mon_off)
    assert re_on == re_off == 0


def _recycle(k, ctx):
    """Before call 12: so many other steps on the same stepper, all kept, that every state slot is claimed."""
    if k != 12:
        return
    m, old = ctx["model"], ctx["f"]
    name, fd, pars, dt, _ = corpus.config_inputs(3, 400)
    other, g, t = schemes.ROS2(m), m.fields_template(**fd), 0.0
    ctx["keep"] = []
    for _ in range(8):
        t, g = other(t, g, dt, ctx["p"])
        ctx["keep"].append(g)
    assert g._device_backing().stepper.nstate < 8
    backing = old._device_backing()
    assert backing is None or not backing.valid()     # the slot behind the old container went to another state


def check_stale_container(backend):
    """(h) The slot behind the container a step was queued from is recycled (eight other steps on the same
    stepper, their results kept, six slots); the next call hands in the old container: not taken from the queue,
    equal to the queue-off run."""
    make = _make("RODASPR", 1e-1)
    on, off = on_and_off(backend, 3, 400, make, before=_recycle)
    plain = drive(backend, 3, 400, make, queue=False)
    assert on.hits[11] == 1 and on.hits[12] == 0, on.hits
    assert_same_run(on, off, "stale container")
    assert_same_run(on, plain, "stale container, undisturbed")          # the other steps changed nothing of this run
