"""Checks of the write-once node-independent Jacobian planes, shared by the CPU emulation suite
(tests/test_uniform_planes.py) and the GPU suite (tests/test_gpu_uniform_planes.py).

The planes of the value table that hold node-independent entries (spec["j_uniform"]) are written by the
first F+J sweep after an upload of a parameter or dx and left alone afterwards
(tf_solver::ju_once).  The reference of every check is the same run on a solver created with
TRIFLOW_J_UNIFORM_ONCE=0, where every sweep writes every plane, as all of them did before: states
and tables are compared BIT FOR BIT, and the full-table sweeps are counted (tf_jacobian_sweeps)."""
import os
from functools import partial

import numpy as np

from oracle import corpus
from triflow_amd import Model
from triflow_amd.compilers import hip_compiler
from triflow_amd.device import DirichletHook
from triflow_amd.ensemble import Ensemble

HOOKS = {"cfg1": DirichletHook(U={0: 1.0, -1: 0.0}), "cfg5": DirichletHook(A={0: 1.0, -1: 1.0}), None: None}


def device_model(name, backend, **kw):
    eqs, dep, pars, helps = corpus.model_args(name)
    compiler = hip_compiler if backend is None else partial(hip_compiler, backend=backend)
    return Model(eqs, dep, pars, helps, compiler=compiler, **kw)


def with_env(pairs, fn):
    """fn() with the environment variables of ``pairs`` set (solvers read their switches when created)."""
    old = {k: os.environ.get(k) for k in pairs}
    os.environ.update({k: str(v) for k, v in pairs.items()})
    try:
        return fn()
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def both(fn, **env):
    """(result with the planes written once, result of the reference run that writes them in every sweep)"""
    return (with_env(dict(env, TRIFLOW_J_UNIFORM_ONCE="1"), fn),
            with_env(dict(env, TRIFLOW_J_UNIFORM_ONCE="0"), fn))


def assert_same(once, every, what):
    """states, tables: bit for bit; the reference run wrote every plane in every sweep"""
    assert len(once["marks"]) == len(every["marks"]) and once["marks"], what
    for k, ((sa, ja), (sb, jb)) in enumerate(zip(once["marks"], every["marks"])):
        assert np.isfinite(sa).all() and np.isfinite(ja).all(), (what, k)
        assert np.array_equal(sa, sb), (what, "state at mark", k)
        assert np.array_equal(ja, jb), (what, "value table at mark", k,
                                        "planes that differ", sorted(set(np.nonzero(ja != jb)[2])))
    assert every["sweeps"]["lean"] == 0, (what, every["sweeps"])
    assert once["sweeps"]["full"] + once["sweeps"]["lean"] == every["sweeps"]["full"], (what, once["sweeps"], every["sweeps"])


def member_inputs(cfg, N, nsys, periodic=None, vary=()):
    name, fd, pars, dt, _ = corpus.config_inputs(cfg, N)
    pars = dict(pars)
    if periodic is not None:
        pars["periodic"] = periodic
    fields = {k: np.repeat(v[None, :], nsys, axis=0) * (1 + 0.01 * np.arange(nsys))[:, None]
              for k, v in fd.items() if k != "x"}
    for key in vary:                                   # one value per member
        pars[key] = pars[key] * (1.0 + 0.25 * np.arange(nsys))
    return name, fd["x"], fields, pars, dt


def stepping_run(backend, cfg, sch, hook, N, nsys=1, periodic=None, vary=(), steps=5, events=None, **opts):
    """`steps` steps of an Ensemble; events: {step index: fn(ens)} run before that step.  Marks (state,
    value table) after steps 3 and `steps`, and after the step that follows every event."""
    name, x, fields, pars, dt = member_inputs(cfg, N, nsys, periodic, vary)
    m = device_model(name, backend)
    events = events or {}

    def run():
        ens = Ensemble(m, x, fields, pars, bool(pars["periodic"]), scheme=sch, hook=HOOKS[hook], **opts)
        marks = []
        for k in range(steps):
            if k in events:
                events[k](ens)
            ens.step(dt)
            if k + 1 in (3, steps) or k in events:
                ens.sync()
                marks.append((ens.state().copy(), ens.solver.get_J().copy()))
        out = dict(marks=marks, sweeps=ens.solver.jacobian_sweeps(), counters=ens.solver.counters(),
                   uniform=sum(ens.solver.model.spec["j_uniform"]), nnz=ens.solver.model.spec["nnz"])
        ens.close()
        return out
    return run


# ------------------------------------------------------------------------------------------ table equality
TABLE_CASES = [
    # (id, config, scheme, hook, N, members, periodic, parameters that differ per member)
    ("film_ros2", 3, "ROS2", None, 1203, 1, True, ()),
    ("film_ros2_clamped", 3, "ROS2", None, 611, 1, False, ()),
    ("film_ros2_members", 3, "ROS2", None, 403, 3, True, ("c", "We")),
    ("film_rodaspr", 3, "RODASPR", None, 803, 1, True, ()),
    ("film_rodaspr_members_clamped", 3, "RODASPR", None, 301, 2, False, ("c", "We")),
    ("diff_theta", 2, "Theta", None, 1500, 1, True, ()),
    ("diff_theta_clamped_members", 2, "Theta", None, 402, 2, False, ("k",)),
    ("stiff_bdf2_hook", 5, "BDF2", "cfg5", 1003, 1, False, ()),
    ("stiff_bdf2_hook_members", 5, "BDF2", "cfg5", 333, 2, False, ("c",)),
    ("stiff_bdf2_periodic", 5, "BDF2", None, 512, 1, True, ()),
]


def check_table_equality(backend, case):
    """After k >= 3 steps the table of the stepping solver (tf_get_J) and its state equal those of a solver that
    writes every plane in every sweep; one full-table sweep, the first."""
    cid, cfg, sch, hook, N, nsys, periodic, vary = case
    once, every = both(stepping_run(backend, cfg, sch, hook, N, nsys, periodic, vary, steps=5, nstate=3))
    assert_same(once, every, cid)
    assert once["sweeps"] == dict(full=1, lean=4), (cid, once["sweeps"])
    expect = {3: (9, 19), 2: (3, 3), 5: None}[cfg]
    if expect:
        assert (once["uniform"], once["nnz"]) == expect, (cid, once["uniform"], once["nnz"])
    else:
        assert 0 < once["uniform"] < once["nnz"], cid


# ------------------------------------------------------------------------------------------ invalidation
def change_dx(ens, factor):
    """dx of every member times ``factor``, and the host constants that depend on it (powers of dx that the
    generated code reads as parameters), as Ensemble.__init__ uploads them."""
    from triflow_amd import codegen
    s, spec = ens.solver, ens.solver.model.spec
    dxs = factor * (ens._x[:, -1] - ens._x[:, 0]) / (ens.N - 1)
    s.set_dx(dxs)
    per_member = [codegen.eval_host_constants(spec, dxs[e], ens._member_pars[e]) for e in range(ens.nsys)]
    for j in range(len(spec["host_consts"])):
        s.set_param(spec["npar_model"] + j, np.array([pm[j] for pm in per_member]))


def check_invalidation_by_uploads(backend):
    """A scalar parameter uploaded between steps, then dx: the table after the next step is complete and equal
    to the reference run's; exactly one full-table sweep per upload (and the first), none otherwise."""
    for cfg, sch, hook, N, par, nsys in ((3, "ROS2", None, 603, "We", 2), (2, "Theta", None, 900, "k", 1),
                                         (5, "BDF2", "cfg5", 407, "Dm", 1)):
        def new_par(ens, par=par):
            k = list(ens.compiled.pars).index(par)
            ens.solver.set_param(k, 1.5 * np.asarray(ens._member_pars[0][k], dtype=float))

        def new_dx(ens):
            change_dx(ens, 1.25)
        once, every = both(stepping_run(backend, cfg, sch, hook, N, nsys, steps=9, events={3: new_par, 6: new_dx},
                                        nstate=3))
        assert_same(once, every, (cfg, sch))
        assert once["sweeps"] == dict(full=3, lean=6), (cfg, sch, once["sweeps"])
        # (both uploads took effect: the uniform planes changed twice)
        tabs = [j for _, j in once["marks"]]
        assert not np.array_equal(tabs[0], tabs[1]) and not np.array_equal(tabs[1], tabs[2]), (cfg, sch)


def check_invalidation_restart(backend):
    """Ensemble.restart copies a state slot: the table stays valid (no full-table sweep), and the steps after it
    leave the table of the reference run."""
    for cfg, sch, hook, N in ((3, "ROS2", None, 603), (5, "BDF2", "cfg5", 407)):
        once, every = both(stepping_run(backend, cfg, sch, hook, N, steps=7, events={4: lambda ens: ens.restart()},
                                        nstate=3))
        assert_same(once, every, (cfg, sch, "restart"))
        assert once["sweeps"] == dict(full=1, lean=6), (cfg, sch, once["sweeps"])


def check_nonuniform_models(backend):
    """A per-node (vector) parameter and an entry that reads x make their entries node dependent: they are written
    by every sweep.  Uploading the vector again invalidates the remaining uniform planes like any upload."""
    # film model with k per node: 6 uniform entries instead of 9, still written once
    name, x, fields, pars, dt = member_inputs(3, 503, 1)
    pars["k"] = pars["k"] * (1.0 + 0.2 * np.cos(2 * np.pi * x / 100))[None, :]
    m = device_model(name, backend)

    def again(ens):
        k = list(ens.compiled.pars).index("k")
        ens.solver.set_param(k, 0.9 * np.asarray(pars["k"]))

    def run():
        ens = Ensemble(m, x, fields, pars, True, scheme="ROS2", nstate=3)
        marks = []
        for k in range(6):
            if k == 3:
                again(ens)
            ens.step(dt)
            if k in (2, 3, 5):
                ens.sync()
                marks.append((ens.state().copy(), ens.solver.get_J().copy()))
        out = dict(marks=marks, sweeps=ens.solver.jacobian_sweeps(), uniform=sum(ens.solver.model.spec["j_uniform"]))
        ens.close()
        return out
    once, every = both(run)
    assert_same(once, every, "vector parameter")
    assert once["uniform"] == 6, once["uniform"]
    assert once["sweeps"] == dict(full=2, lean=4), once["sweeps"]

    # an entry that reads x: k * x * dxxU has no uniform entry, k * dxxU + x * U keeps the off-diagonal ones
    compiler = hip_compiler if backend is None else partial(hip_compiler, backend=backend)
    for eq, nuni in (("k * x * dxxU", 0), ("k * dxxU - x * U", 2)):
        N = 400
        xs = np.linspace(0.5, 1.5, N)
        U = (1 + 0.3 * np.cos(7 * xs))[None, :]

        def run_x(eq=eq):
            mx = Model(eq, "U", "k", compiler=compiler)
            ens = Ensemble(mx, xs, dict(U=U), dict(k=1e-3, periodic=False), False, scheme="Theta", nstate=3)
            marks = []
            for k in range(5):
                if k == 3:
                    ens.solver.set_param(0, 2e-3)
                ens.step(1e-2)
                if k in (2, 3, 4):
                    ens.sync()
                    marks.append((ens.state().copy(), ens.solver.get_J().copy()))
            out = dict(marks=marks, sweeps=ens.solver.jacobian_sweeps(), uniform=sum(ens.solver.model.spec["j_uniform"]))
            ens.close()
            return out
        once, every = both(run_x)
        assert_same(once, every, eq)
        assert once["uniform"] == nuni, (eq, once["uniform"])
        assert once["sweeps"] == dict(full=2, lean=3), (eq, once["sweeps"])


# ------------------------------------------------------------------------------------------ rescue path
def check_rescue_path(backend):
    """The forced 4-node plan of check_unstable_factorisation_recovers (dispersive scalar equation): the child solver
    on longer chunks receives the complete table -- also when the sweep before the transfer skipped the uniform
    planes (kdv: the dxxxU entries) -- and gives the same solution as with the switch off."""
    from tests.parity_cases import bound_solver
    name, N, c = "kdv", 203, 0.1
    m = device_model(name, backend)
    fd = corpus.synthetic_fields(name, N, seed=7, periodic=True, length=N * 5e-3)
    pars = corpus.synthetic_pars(name, N, True)
    rhs = np.random.default_rng(5).standard_normal(N)

    def run():
        # (nstate: another key of the model's solver cache than the other run's)
        s = bound_solver(m, fd, pars, m1=4, m_upper=2, nstate=4 + int(os.environ["TRIFLOW_J_UNIFORM_ONCE"]))
        out = []
        s.eval(0, with_j=True)                    # full table
        s.eval(0, with_j=True)                    # (with the switch on: the uniform planes are left alone)
        s.factor(c)
        out.append(s.solve(rhs)[0].copy())        # breaks down on 4-node chunks: the child gets the table
        s.set_dx(1.1 * (fd["x"][-1] - fd["x"][0]) / (N - 1))
        s.eval(0, with_j=True)
        s.eval(0, with_j=True)
        s.factor(c)
        out.append(s.solve(rhs)[0].copy())
        res = dict(x=out, table=s.get_J().copy(), replans=s.counters()["replans"], sweeps=s.jacobian_sweeps(),
                   uniform=sum(s.model.spec["j_uniform"]))
        return res
    once, every = both(run)
    assert once["replans"] >= 1 and once["uniform"] > 0, (once["replans"], once["uniform"])
    assert once["sweeps"] == dict(full=2, lean=2) and every["sweeps"] == dict(full=4, lean=0), (once["sweeps"], every["sweeps"])
    assert np.array_equal(once["table"], every["table"])
    for a, b in zip(once["x"], every["x"]):
        assert np.isfinite(a).all() and np.array_equal(a, b)
    assert not np.array_equal(once["x"][0], once["x"][1])


# ------------------------------------------------------------------------------------------ graph replay
def check_graph_replay(backend, N=2000):
    """Captured steps (TRIFLOW_GRAPHS=1) hold the kernel arguments, the flag among them: steps, a parameter
    upload, more steps, another upload, more steps -- equal to the run without graphs, tables included."""
    for cfg, sch, hook, par in ((3, "ROS2", None, "We"), (2, "Theta", None, "k"), (5, "BDF2", "cfg5", "Dm")):
        def upload(factor, ens, par=par):
            k = list(ens.compiled.pars).index(par)
            ens.solver.set_param(k, factor * np.asarray(ens._member_pars[0][k], dtype=float))
        events = {5: partial(upload, 1.5), 9: partial(upload, 0.75), 13: partial(upload, 1.25)}
        runs = {}
        for graphs in ("1", "0"):
            for switch in ("1", "0"):
                runs[graphs, switch] = with_env(
                    dict(TRIFLOW_GRAPHS=graphs, TRIFLOW_J_UNIFORM_ONCE=switch),
                    stepping_run(backend, cfg, sch, hook, N, steps=17, events=events, nstate=3, refine=0))
        assert_same(runs["1", "1"], runs["0", "0"], (cfg, sch, "graphs + once against neither"))
        assert_same(runs["1", "1"], runs["1", "0"], (cfg, sch, "graphs"))
        assert_same(runs["0", "1"], runs["0", "0"], (cfg, sch, "no graphs"))
        assert runs["1", "1"]["sweeps"] == dict(full=4, lean=13), runs["1", "1"]["sweeps"]


# ------------------------------------------------------------------------------------------ two factorisations
def check_step_doubling_trial(backend):
    """The step-doubling trial of the config 2 model (two resident factorisations, coarse and fine steps queued
    back to back): the states and the error estimate of the run with the switch off."""
    from triflow_amd.tableaux import TABLEAUX
    name, fd, pars, dt, _ = corpus.config_inputs(2, 1500)
    m = device_model(name, backend)
    tab = TABLEAUX["ROS2"]
    for desc in (dict(kind="theta", theta=1.0),
                 dict(kind="row", alpha=tab.alpha, gamma=tab.gamma, b=tab.b, hook_after=True)):
        def run():
            ens = Ensemble(m, fd["x"], {"U": fd["U"][None, :]}, pars, True, scheme="Theta", nstate=4)
            s = ens.solver
            errs, marks = [], []
            for trial in range(3):
                if trial == 2:
                    s.set_param(0, 2 * pars["k"])
                errs.append(np.array(s.step_doubling(0, 1, 2, 3, dt, 10, desc)).copy())
                marks.append((s.get_state(1).copy(), s.get_J().copy()))
                marks.append((s.get_state(3).copy(), s.get_J().copy()))
                s.copy_state(1, 0)
            out = dict(marks=marks, errs=errs, sweeps=s.jacobian_sweeps(), counters=s.counters())
            ens.close()
            return out
        once, every = both(run)
        assert_same(once, every, desc["kind"])
        for a, b in zip(once["errs"], every["errs"]):
            assert np.array_equal(a, b)
        assert once["counters"] == every["counters"]
        assert once["sweeps"] == dict(full=2, lean=31), once["sweeps"]
