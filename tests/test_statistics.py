"""Device statistics on the CPU: the fold and the walk through the host harness (tests/stat_host: the
generated statistic block and csrc/tf_stat.h compiled with g++) against the recurrences in NumPy, the
identities that follow from them, NaN and ties, lowering, validation, rollback and the host side of a set
(which statistics are due, what happens to the accumulators when the solver changes)."""
import math

import numpy as np
import pytest
from sympy import lambdify

from oracle import corpus
from oracle import numpy_path as ora
from tests.stat_host import build_stat_host as host
from triflow_amd import Model, codegen, compilers, probes, statistics
from triflow_amd.codegen import UnsupportedExpression
from triflow_amd.simulation import Simulation
from triflow_amd.statistics import MAX_STATISTICS, STATISTIC_KINDS

_MODELS = {}


def _model(name):
    if name not in _MODELS:
        _MODELS[name] = Model(*corpus.model_args(name), hold_compilation=True)
    return _MODELS[name]


_FUNCS = {}


def numpy_nodes(model, exprs, fields, pars):
    """The per-node values NumPy computes for one state (tests/test_gpu_recorders.py::reference_rows,
    pool "sample"): the lambdified discretised expressions with the reference's module dictionary, on
    the ghost-padded views of the reference."""
    if (id(model), tuple(exprs)) not in _FUNCS:
        disc = [probes.discretise(model, e) for e in exprs]
        _FUNCS[id(model), tuple(exprs)] = lambdify(model._symbolic_args, disc, modules=ora._lambdify_modules())
    func = _FUNCS[id(model), tuple(exprs)]
    inputs = [np.asarray(fields["x"])] + [np.asarray(fields[k]) for k in model._dep_vars] + \
        [pars[k] for k in model._pars] + [pars["periodic"]]
    env, N, _, _ = ora.stencil_views(model, *inputs)
    with np.errstate(all="ignore"):
        vals = func(*[env[k] for k in model._args])
    return [np.array(np.broadcast_to(np.asarray(v, dtype=float), (N,))) for v in vals]


def numpy_fold(kind, samples):
    """The recurrences of the statistics over ``samples = [(t, v [N]), ...]``:
    the accumulator planes [planes][N] after the last of them."""
    a0 = a1 = None
    with np.errstate(all="ignore"):
        for k, (t, v) in enumerate(samples, 1):
            kk = float(k)
            if k == 1:
                a0 = np.array(v)
                a1 = np.zeros_like(v) if kind == "var" else np.full_like(v, t)
            elif kind == "mean":
                a0 = a0 + (v - a0) / kk
            elif kind == "var":
                d = v - a0
                m = a0 + d / kk
                a1 = a1 + d * (v - m)
                a0 = m
            else:
                up = kind in ("max", "argmax")
                better = np.where(up, v > a0, v < a0)
                if kind in ("max", "min"):        # NaN wins
                    a0 = np.where(np.isnan(a0), a0, np.where(np.isnan(v) | better, v, a0))
                else:                             # the first sample at the extremum, the first NaN
                    take = ~np.isnan(a0) & (np.isnan(v) | better)
                    a0, a1 = np.where(take, v, a0), np.where(take, t, a1)
    return np.array([a0, a1]) if kind in ("var", "argmax", "argmin") else np.array([a0])


def value_of(kind, planes, n):
    if kind == "var":
        return planes[1] / float(n)
    return planes[1] if kind in ("argmax", "argmin") else planes[0]


CASES = [("M3_film", True, ["h", "We * h * dxxxh", "x", "c"]),
         ("M1_advdiff", False, ["U", "c * dxU**2", "x", "k"])]
# chunks of 50 | 17 17 16 | 8 7 7 7 7 7 7 and of 53 | 18 18 17 | 9 9 9 9 9 8 nodes: one chunk, chunks of
# different lengths, lengths that are no multiple of TF_PROBE_SEG = 8, a last segment of one node (17, 9)
GRIDS = [(50, 1), (50, 3), (50, 7), (53, 1), (53, 3), (53, 6)]
NSTATES = 7


def _states(name, N, periodic):
    """Seven synthetic states of one grid: the seeded perturbation differs from state to state."""
    return [(0.25 * s, corpus.synthetic_fields(name, N, seed=s, periodic=periodic)) for s in range(NSTATES)]


def laid_out(h, states):
    return [(t, h.state(fields)) for t, fields in states]


def harness_fold(h, which, kind, laid):
    """``laid``: (t, state of the harness) per sample."""
    acc = h.planes(kind)
    for k, (t, state) in enumerate(laid, 1):
        h.update(which, kind, k, t, state, acc)
    return h.natural(acc)


@pytest.mark.parametrize("name,periodic,exprs", CASES, ids=[c[0] for c in CASES])
@pytest.mark.parametrize("N,P", GRIDS)
def test_accumulators_bit_identical_to_the_recurrences_in_numpy(name, periodic, exprs, N, P):
    model = _model(name)
    pars = corpus.synthetic_pars(name, N, periodic)
    states = _states(name, N, periodic)
    h = host.Harness(model, exprs, states[0][1]["x"], pars, periodic, P)
    nodes = [numpy_nodes(model, exprs, f, pars) for _, f in states]
    laid = laid_out(h, states)
    for which, e in enumerate(exprs):
        samples = [(t, nodes[i][which]) for i, (t, _) in enumerate(states)]
        for kind in STATISTIC_KINDS:
            got = harness_fold(h, which, kind, laid)
            want = numpy_fold(kind, samples)
            assert got.shape == want.shape, (e, kind)
            assert got.tobytes() == want.tobytes(), (e, kind, np.abs(got - want).max())


def test_identities_that_follow_from_the_recurrences():
    name, periodic, exprs = CASES[0]
    model, N, P = _model(name), 53, 6
    pars = corpus.synthetic_pars(name, N, periodic)
    states = _states(name, N, periodic)
    h = host.Harness(model, exprs, states[0][1]["x"], pars, periodic, P)
    n, laid = len(states), laid_out(h, states)
    # constant in time: d = 0 in every update
    for which, const in ((2, states[0][1]["x"]), (3, np.full(N, pars["c"]))):
        var = harness_fold(h, which, "var", laid)
        assert np.array_equal(var[1], np.zeros(N)) and np.array_equal(var[0], const)
        assert np.array_equal(harness_fold(h, which, "mean", laid)[0], const)
    for which in (0, 1):
        v = np.array([numpy_nodes(model, exprs, f, pars)[which] for _, f in states])
        mean = harness_fold(h, which, "mean", laid)[0]
        top, low = harness_fold(h, which, "max", laid)[0], harness_fold(h, which, "min", laid)[0]
        assert np.array_equal(top, v.max(axis=0)) and np.array_equal(low, v.min(axis=0))
        assert (top >= mean).all() and (mean >= low).all()
        # every update rounds three times, each by at most 2**-53 * 2 max|v|, and passes the error of
        # the mean before it on with the factor 1 - 1/k <= 1
        exact = np.array([math.fsum(v[:, j]) / n for j in range(N)])
        bound = 5 * n * 2.0 ** -53 * np.abs(v).max(axis=0)
        err = np.abs(mean - exact)
        print(exprs[which], "mean: worst error / bound %.3g" % (err / bound).max())
        assert (err <= bound).all()
        var = value_of("var", harness_fold(h, which, "var", laid), n)
        assert (var >= 0).all() and np.allclose(var, v.var(axis=0), rtol=1e-10, atol=0)


def _plain_harness(N=53, P=6):
    model = _model("M1_advdiff")
    x = np.linspace(0.0, 3.0, N)
    return host.Harness(model, ["U"], x, dict(k=.1, c=.2, periodic=False), False, P), x


def test_nan_at_one_node_in_one_sample():
    h, x = _plain_harness()
    rng = np.random.default_rng(5)
    values = rng.standard_normal((5, x.size))
    clean = [(0.5 * i, dict(x=x, U=values[i])) for i in range(5)]
    values = values.copy()
    values[2, 20] = np.nan                                  # sample 3 of 5
    states = [(0.5 * i, dict(x=x, U=values[i])) for i in range(5)]
    others = np.arange(x.size) != 20
    laid, laid_clean = laid_out(h, states), laid_out(h, clean)
    for kind in STATISTIC_KINDS:
        got, ref = harness_fold(h, 0, kind, laid), harness_fold(h, 0, kind, laid_clean)
        assert got[:, others].tobytes() == ref[:, others].tobytes(), kind       # the neighbours: untouched
        assert got.tobytes() == numpy_fold(kind, [(t, f["U"]) for t, f in states]).tobytes(), kind
        if kind in ("argmax", "argmin"):
            assert np.isnan(got[0, 20]) and got[1, 20] == states[2][0]
        else:
            assert np.isnan(got[:, 20]).all(), kind
    for upto in (3, 4):                                     # ... from sample 3 on
        for kind in ("max", "min", "mean"):
            assert np.isnan(harness_fold(h, 0, kind, laid[:upto])[0, 20])
    assert not np.isnan(harness_fold(h, 0, "mean", laid[:2])[0, 20])


def test_ties_go_to_the_earlier_sample():
    h, x = _plain_harness()
    base = np.cos(x)
    states = [(1.0 + i, dict(x=x, U=base + (i % 2))) for i in range(5)]        # samples 2 and 4 are equal
    laid = laid_out(h, states)
    top, low = harness_fold(h, 0, "argmax", laid), harness_fold(h, 0, "argmin", laid)
    assert np.array_equal(top[0], base + 1) and np.array_equal(top[1], np.full(x.size, 2.0))
    assert np.array_equal(low[0], base) and np.array_equal(low[1], np.full(x.size, 1.0))


# ---- lowering ----------------------------------------------------------------------------------
def test_statistic_block_and_spec():
    model = _model("M3_film")
    disc = [probes.discretise(model, e) for e in ("h", "dxh * k**3", "x * q")]
    block, spec = codegen.lower_statistics(model, disc)
    assert "#define TF_NSTAT 3" in block and "#define TF_STAT_USES_X 1" in block and "#define TF_NSTAT_HC 1" in block
    assert "tf_eval_stat(int k," in block and spec["nstat"] == 3
    rblock, rspec = codegen.lower_records(model, disc)
    assert rspec["host_consts"] == spec["host_consts"] and rspec["uses_x"] == spec["uses_x"]
    cases = [ln for ln in rblock.splitlines() if ln.startswith("    case ")]
    assert len(cases) == 3 and cases == [ln for ln in block.splitlines() if ln.startswith("    case ")]
    with pytest.raises(UnsupportedExpression, match="Heaviside"):
        codegen.lower_statistics(model, [probes.discretise(model, "Heaviside(h - 1)")])


def test_the_statistic_kernel_follows_the_table():
    with open(compilers.CSRC + "/tf_args.h") as f:
        text = f.read()
    assert 'TF_KERNEL_NAMES_STAT { "tfk_stat" }' in text and "TFK_STAT = TFK_COUNT" in text
    assert "tf_rt_stat.cpp" in compilers.RUNTIME_SOURCES        # (the code objects: tests/test_observer_objects.py)
    assert statistics.StatisticSet.kind == "stat"
    with pytest.raises(ValueError, match="kind of observer"):
        compilers.build_observer_code_object(_model("M2_diff"), "", "statistic")


# ---- validation --------------------------------------------------------------------------------
def _sim(name="M2_diff", N=50):
    model = _model(name)
    fields = corpus.synthetic_fields(name, N)
    return Simulation(model, fields, corpus.synthetic_pars(name, N, True), dt=1e-3, time_stepping=False)


@pytest.mark.parametrize("kwargs,match", [
    (dict(stat="median"), "stat"),
    (dict(stat="sum"), "stat"),
    (dict(every=0), "every"),
    (dict(every=1.5), "every"),
    (dict(every=True), "every"),
    (dict(nodes=slice(None, None, -1)), "step"),
    (dict(nodes=slice(None, None, 0)), "nodes"),
    (dict(nodes=5), "slice"),
    (dict(nodes=[1, 2]), "slice"),
    (dict(nodes=slice(10, 10)), "no node"),
    (dict(nodes=slice(60, None)), "no node"),
])
def test_validation_errors(kwargs, match):
    with pytest.raises(ValueError, match=match) as err:
        _sim().add_statistic("s", "U", **kwargs)
    assert "statistic" in str(err.value)


@pytest.mark.parametrize("expr", ["U *", "foo * U", "bar(U)", "dxk", 3])
def test_badly_formed_or_unknown_symbol(expr):
    with pytest.raises(ValueError, match="badly formated"):
        _sim().add_statistic("s", expr)


def test_wider_stencil_than_the_window_names_the_limit():
    with pytest.raises(UnsupportedExpression, match=r"half width 1\b"):
        _sim("M2_diff").add_statistic("s", "dxxxU", stat="max")


def test_heaviside_is_refused():
    with pytest.raises(UnsupportedExpression, match="Heaviside"):
        _sim().add_statistic("s", "Heaviside(U - 1) * U")


def test_duplicate_names_removal_and_the_limit():
    ss = statistics.StatisticSet(_model("M2_diff"), 50)
    ss.add("a", "U", stat="var", every=3, nodes=slice(None, None, 4))
    with pytest.raises(ValueError, match="statistic named 'a' exists already"):
        ss.add("a", "dxU")
    ss.add("b", "dxU")
    assert ss.names == ["a", "b"] and len(ss.expressions()) == 2
    ss.remove("a")
    assert ss.names == ["b"]
    with pytest.raises(KeyError):
        ss.remove("a")
    with pytest.raises(KeyError):
        ss.reset("a")
    for call in ("remove_statistic", "reset_statistic"):
        with pytest.raises(KeyError):
            getattr(_sim(), call)("nope")
    n, x, v = ss.series(per_system=False)["b"]
    assert n == 0 and x is None and v.shape == (50,) and np.isnan(v).all()
    assert _sim().statistics == {}
    for k in range(MAX_STATISTICS - 1):
        ss.add("s%d" % k, "U", stat=STATISTIC_KINDS[k % 6])
    assert len(ss.names) == MAX_STATISTICS == 64 and len(ss.expressions()) == 2
    with pytest.raises(ValueError, match="at most 64 statistics"):
        ss.add("one more", "U")


# ---- the host side of a set ----------------------------------------------------------------------
class _FakeStepper:
    class compiled:
        pars = ["k"]
    solver = None

    def bind(self, fields, pars):
        pass

    def acquire(self, fields):
        return 0


def test_statistic_that_cannot_run_is_not_kept(monkeypatch):
    def fail(self, solver):
        raise UnsupportedExpression("the stat kernels need more registers than a wavefront has")
    import triflow_amd.simulation as simulation
    monkeypatch.setattr(simulation, "stepper_for", lambda *a, **k: _FakeStepper())
    sim = _sim()
    rs = sim._statistics = statistics.StatisticSet(sim.model, 50)
    rs.add("kept", "U", stat="max")
    kept = rs._items[0]
    kept.n, kept.last, kept.origin, kept.held = 3, sim.i, sim.i, np.arange(50.0).reshape(1, 1, 50)
    monkeypatch.setattr(statistics.StatisticSet, "_bind", fail)
    with pytest.raises(UnsupportedExpression):
        sim.add_statistic("s", "U", stat="var")
    assert list(sim.statistics) == ["kept"] and sim._statistics.names == ["kept"]
    n, x, v = sim.statistics["kept"]
    assert n == 3 and np.array_equal(v, np.arange(50.0))
    sim.remove_statistic("kept")
    with pytest.raises(UnsupportedExpression):
        sim.add_statistic("s", "U")
    assert sim.statistics == {} and sim._statistics.names == []


class _Handle:
    """Stands in for _capi.DeviceStat: plane 0 counts the updates, the calls are kept."""

    def __init__(self, solver):
        self.solver, self.calls, self.planes = solver, [], {}

    def set_x(self, x):
        pass

    def update(self, k, slot, n, t):
        self.calls.append(("update", k, n, t))
        self.planes[k] = self.planes.get(k, np.zeros((2, 1, 50))) + 1.0

    def fetch(self, k):
        self.calls.append(("fetch", k))
        return self.planes[k].copy()

    def load(self, k, planes):
        self.calls.append(("load", k))
        self.planes[k] = np.array(planes)

    def close(self):
        pass


class _Solver:
    nsys, N = 1, 50

    class model:
        spec = dict(uses_x=0)


def _fake_set():
    ss = statistics.StatisticSet(_model("M2_diff"), 50)
    bounds = {}

    def bind(solver):
        if id(solver) not in bounds:
            bounds[id(solver)] = statistics._Bound(_Handle(solver), dict(host_consts=[]))
        return bounds[id(solver)]
    ss._bind = bind
    return ss, bounds


def test_only_statistics_that_are_due_are_launched_and_reset_starts_over():
    ss, bounds = _fake_set()
    x = np.linspace(0, 1, 50)
    solver = _Solver()
    ss.add("every1", "U", nodes=slice(7, 9))
    ss.record(solver, 0, 0.4, 4, x, [[1.0]])
    ss.add("every3", "U", stat="argmax", every=3, nodes=slice(7, 8))
    bounds.clear()                                         # (add closed the handles: a new one is bound)
    ss.record(solver, 0, 0.4, 4, x, [[1.0]])               # (sample 1 of the new one only)
    handle = bounds[id(solver)].handle
    assert handle.calls == [("update", 1, 1, 0.4)]
    for key in range(5, 12):
        ss.record(solver, 0, 0.1 * key, key, x, [[1.0]])
    ups = [c[1:3] for c in handle.calls if c[0] == "update"]
    assert ups == [(1, 1), (0, 2), (0, 3), (0, 4), (1, 2), (0, 5), (0, 6), (0, 7), (1, 3), (0, 8)]
    assert handle.calls[1] == ("load", 0)                  # every1's sample 1 came back when the set changed
    s = ss.series(per_system=False)
    assert s["every1"][0] == 8 and s["every3"][0] == 3
    assert np.array_equal(s["every1"][1], x[7:9]) and s["every1"][2].shape == (2,)
    ss.reset("every1")
    assert ss.series(per_system=False)["every1"][0] == 0
    ss.record(solver, 0, 1.1, 11, x, [[1.0]])              # the state of the last sample: not again
    ss.record(solver, 0, 1.2, 12, x, [[1.0]])
    assert handle.calls[-1] == ("update", 0, 1, 1.2) and ss.series(per_system=False)["every1"][0] == 1
    assert ("load", 0) not in handle.calls[2:]             # a reset moves nothing


def test_a_change_of_solver_takes_the_accumulators_along():
    ss, bounds = _fake_set()
    x = np.linspace(0, 1, 50)
    first, second = _Solver(), _Solver()
    ss.add("m", "U", stat="var")
    for key in range(4):
        ss.record(first, 0, 0.1 * key, key, x, [[1.0]])
    for key in range(4, 7):
        ss.record(second, 0, 0.1 * key, key, x, [[1.0]])
    a, b = bounds[id(first)].handle, bounds[id(second)].handle
    assert a.calls[-1] == ("fetch", 0) and b.calls[0] == ("load", 0)
    assert [c[2] for c in b.calls if c[0] == "update"] == [5, 6, 7]
    n, _, v = ss.series(per_system=False)["m"]
    assert n == 7 and np.array_equal(v, np.full(50, 7.0) / 7.0)

    class Other(_Solver):
        N = 60
    ss2 = statistics.StatisticSet(_model("M2_diff"), 50)
    ss2.add("m", "U")
    with pytest.raises(ValueError, match="laid out for 50 nodes"):
        ss2.record(Other(), 0, 0.0, 0, np.linspace(0, 1, 60), [[1.0]])
