"""Device extrema on the CPU: the rule, the walk and the scan arithmetic through the host harness
(tests/extrema_host: the generated extrema block and csrc/tf_extrema.h compiled with g++) against the NumPy
referee (tests/extrema_cases.py) -- exactly --, the referee itself against scipy, lowering, validation,
rollback, the refinement and the host side of a set."""
import re

import numpy as np
import pytest

from oracle import corpus
from tests import extrema_cases as cases
from tests.extrema_host import build_extrema_host as host
from tests.test_statistics import numpy_nodes
from triflow_amd import Model, _capi, codegen, compilers, extrema, probes
from triflow_amd.codegen import UnsupportedExpression
from triflow_amd.extrema import MAX_COUNT, MAX_EXTREMA
from triflow_amd.simulation import Simulation

_MODELS = {}


def _model(name):
    if name not in _MODELS:
        _MODELS[name] = Model(*corpus.model_args(name), hold_compilation=True)
    return _MODELS[name]


# (model, periodic, expressions, the field that expression 0 is)
CASES = [("M3_film", True, ["h", "We * h * dxxxh", "x"], "h"),
         ("M1_advdiff", False, ["U", "c * dxU**2"], "U")]
# chunks of 3 | 50 | 9 9 9 9 9 8 | 4 (16 of them) | 16 (4 of them) | 5 5 4 ... (257 chunks: two workgroups,
# the second with one chunk) | 17 x 7, 16 x 253 (260 chunks) | 5 x 76, 4 x 524 (600 chunks: three workgroups)
GRIDS = [(3, 1), (50, 1), (53, 6), (64, 16), (64, 4), (1030, 257), (4167, 260), (2476, 600)]
_HARNESS = {}


def _harness(name, periodic, exprs, N, P):
    key = (name, periodic, N, P)
    if key not in _HARNESS:
        model = _model(name)
        pars = corpus.synthetic_pars(name, N, periodic)
        fields = corpus.synthetic_fields(name, N, seed=1, periodic=periodic)
        _HARNESS[key] = (host.Harness(model, exprs, fields["x"], pars, periodic, P), fields, pars)
    return _HARNESS[key]


def _check(h, which, fields, v, periodic, kind="max", threshold=None, max_count=MAX_COUNT, label=""):
    n, g, tri = h.run(which, fields, kind, threshold, max_count)
    rg, rt = cases.referee(v, kind, periodic, threshold)
    k = min(rg.size, max_count)
    assert n == rg.size, (label, n, rg.size)
    assert np.array_equal(g, rg[:k]), (label, g, rg[:k])
    assert tri.tobytes() == rt[:k].tobytes(), label
    return n


def test_the_referee_is_argrelextrema():
    from scipy.signal import argrelextrema
    for N in (3, 50, 4167):
        for v in (cases.sawtooth(N), cases.random_field(N), np.ones(N), cases.single_crest(N, 0),
                  cases.single_crest(N, N - 1)):
            for periodic in (True, False):
                for kind, cmp in (("max", np.greater), ("min", np.less)):
                    (ref,) = argrelextrema(v, cmp, mode="wrap" if periodic else "clip")
                    g, tri = cases.referee(v, kind, periodic)
                    assert np.array_equal(g, ref), (N, periodic, kind)
                    assert np.array_equal(tri[:, 1], v[g]) and np.array_equal(tri[:, 0], v[g - 1])
                    assert np.array_equal(tri[:, 2], v[(g + 1) % N])
    # where the rule says more than scipy does: an infinite node is no extremum, a threshold
    v = np.array([0.0, np.inf, 0.0, 1.0, 0.5, 3.0, 0.0, -np.inf, 0.0])
    assert list(cases.referee(v, "max", False)[0]) == [3, 5]
    assert list(cases.referee(v, "max", False, threshold=1.0)[0]) == [5]
    assert list(cases.referee(v, "min", False)[0]) == [2, 4] and list(cases.referee(v, "min", False, 0.5)[0]) == [2]


@pytest.mark.parametrize("name,periodic,exprs,var", CASES, ids=[c[0] for c in CASES])
@pytest.mark.parametrize("N,P", GRIDS)
def test_walk_against_the_referee(name, periodic, exprs, var, N, P):
    """Crafted fields through expression 0 (the field itself), then every expression of the block on the
    synthetic state: n, every g and every triple bit for bit, both kinds."""
    h, fields, pars = _harness(name, periodic, exprs, N, P)
    nan_beside = cases.single_crest(N, N // 2)
    nan_beside[N // 2 - 1] = np.nan                       # a would-be crest with a NaN neighbour
    crafted = dict(sawtooth=cases.sawtooth(N), random=cases.random_field(N), constant=np.full(N, 1.25),
                   crest0=cases.single_crest(N, 0), crestN1=cases.single_crest(N, N - 1), nan=nan_beside)
    found = {}
    for label, v in crafted.items():
        f = dict(fields, **{var: v})
        for kind in ("max", "min"):
            found[label, kind] = _check(h, 0, f, v, periodic, kind, label=(label, kind, N, P))
    assert found["constant", "max"] == found["constant", "min"] == 0
    assert found["sawtooth", "max"] == (N // 2 if periodic or N % 2 else N // 2 - 1)
    assert found["crest0", "max"] == found["crestN1", "max"] == (1 if periodic else 0)
    assert found["nan", "max"] == 0
    if N > 3:
        assert found["random", "max"] > N // 5
    nodes = numpy_nodes(_model(name), exprs, fields, pars)
    for which in range(len(exprs)):
        for kind in ("max", "min"):
            _check(h, which, fields, nodes[which], periodic, kind, label=(exprs[which], kind, N, P))


@pytest.mark.parametrize("periodic", [True, False])
def test_a_crest_at_either_end_on_both_kinds_of_grid(periodic):
    """Node 0 and node N - 1 are extrema of a periodic grid only (through the same model: the layout's
    flag alone decides)."""
    name, _, exprs, var = CASES[1]
    for N, P in ((50, 1), (53, 6), (1030, 257)):
        h, fields, _ = _harness(name, periodic, exprs, N, P)
        for at in (0, N - 1):
            v = cases.single_crest(N, at)
            n, g, tri = h.run(0, dict(fields, U=v), "max")
            assert (n, list(g)) == ((1, [at]) if periodic else (0, [])), (N, P, at)
            if periodic:
                assert tri.tobytes() == np.array([[v[at - 1], v[at], v[(at + 1) % N]]]).tobytes()
            _check(h, 0, dict(fields, U=-v), -v, periodic, "min")


def test_threshold_on_both_kinds_and_non_finite_nodes():
    name, periodic, exprs, var = CASES[0]
    N, P = 1030, 257
    h, fields, _ = _harness(name, periodic, exprs, N, P)
    v = cases.random_field(N)
    f = dict(fields, h=v)
    everything = _check(h, 0, f, v, periodic, "max")
    above = _check(h, 0, f, v, periodic, "max", threshold=1.05)
    below = _check(h, 0, f, v, periodic, "min", threshold=0.95)
    assert 0 < above < everything and 0 < below < everything
    crest = float(np.max(v))
    assert _check(h, 0, f, v, periodic, "max", threshold=crest) == 0           # strictly greater
    assert _check(h, 0, f, v, periodic, "max", threshold=np.nextafter(crest, 0)) == 1
    v = cases.random_field(N)
    g, _ = cases.referee(v, "max", periodic)
    v[g[3]], v[g[5]], v[g[7] + 1] = np.inf, np.nan, np.nan
    assert _check(h, 0, dict(fields, h=v), v, periodic, "max") < g.size
    assert _check(h, 0, dict(fields, h=v), v, periodic, "min") > 0
    lib = h.lib
    assert lib.extrema_host_is(0, -np.inf, 0.0, 1.0, 0.0) == 1 and lib.extrema_host_is(0, -np.inf, 0.0, np.inf, 0.0) == 0
    assert lib.extrema_host_is(0, -np.inf, -np.inf, 1.0, -np.inf) == 1          # infinite neighbours compare
    assert lib.extrema_host_is(0, -np.inf, 1.0, 1.0, 0.0) == 0 and lib.extrema_host_is(0, -np.inf, 0.0, 1.0, 1.0) == 0
    assert lib.extrema_host_is(1, np.inf, 1.0, 0.0, 1.0) == 1 and lib.extrema_host_is(1, np.inf, 1.0, -np.inf, 1.0) == 0
    assert lib.extrema_host_is(0, -np.inf, np.nan, 1.0, 0.0) == 0 and lib.extrema_host_is(1, np.inf, 1.0, 0.0, np.nan) == 0


@pytest.mark.parametrize("N,P", [(53, 6), (1030, 257), (2476, 600)])
def test_max_count_smaller_than_n_keeps_the_first(N, P):
    name, periodic, exprs, var = CASES[0]
    h, fields, _ = _harness(name, periodic, exprs, N, P)
    v = cases.random_field(N)
    f = dict(fields, h=v)
    full = _check(h, 0, f, v, periodic, "max")
    walks_full = h.walks
    for mc in (1, 7, full - 1, full, full + 1):
        assert _check(h, 0, f, v, periodic, "max", max_count=mc) == full    # (n is still the total)
        assert h.walks <= walks_full
    _check(h, 0, f, v, periodic, "max", max_count=1)
    assert h.walks == 1                                    # chunks whose entries lie past max_count do not walk again


# ---- lowering ----------------------------------------------------------------------------------
def test_extrema_block_and_spec():
    model = _model("M3_film")
    disc = [probes.discretise(model, e) for e in ("h", "dxh * k**3", "x * q")]
    block, spec = codegen.lower_extrema(model, disc)
    assert "#define TF_NEXT 3" in block and "#define TF_EXT_USES_X 1" in block and "#define TF_NEXT_HC 1" in block
    assert "tf_eval_extrema(int k," in block and spec["next"] == 3
    rblock, rspec = codegen.lower_records(model, disc)
    assert rspec["host_consts"] == spec["host_consts"] and rspec["uses_x"] == spec["uses_x"]
    lines = [ln for ln in rblock.splitlines() if ln.startswith("    case ")]
    assert len(lines) == 3 and lines == [ln for ln in block.splitlines() if ln.startswith("    case ")]
    with pytest.raises(UnsupportedExpression, match="Heaviside"):
        codegen.lower_extrema(model, [probes.discretise(model, "Heaviside(h - 1)")])


def test_sets_that_differ_in_launch_arguments_share_a_block():
    a = extrema.ExtremaSet(_model("M2_diff"), 50)
    a.add("p", "U", kind="max", threshold=None, max_count=256, every=1)
    a.add("q", "dxU", kind="min")
    b = extrema.ExtremaSet(_model("M2_diff"), 50)
    b.add("r", "U", kind="min", threshold=0.25, max_count=16, every=7, refine=False)
    b.add("s", "dxU", kind="max", threshold=-1.0, max_count=8192, capacity=3)
    b.add("t", "U", kind="max")                            # the same expression again: the same case
    assert len(b.expressions()) == 2
    assert a._lower(0)[0] == b._lower(0)[0]
    assert a._lower(0)[1] == b._lower(0)[1]


def test_the_extrema_kernels_follow_the_table():
    with open(compilers.CSRC + "/tf_args.h") as f:
        text = f.read()
    # what the tests of the other observers pin stays as it was
    assert 'TF_KERNEL_NAMES_STAT { "tfk_stat" }' in text and "TFK_STAT = TFK_COUNT" in text
    assert re.search(r"TFK_PROBE_FINAL,\s*TFK_RECORD, TFK_COUNT", text)
    assert 'TF_KERNEL_NAMES_SPECTRUM { "tfk_spectrum_partial", "tfk_spectrum_final" }' in text
    assert 'TF_KERNEL_NAMES_EXTREMA { "tfk_extrema_count", "tfk_extrema_write" }' in text
    assert int(re.search(r"#define TF_EXT_MAX_COUNT (\d+)", text).group(1)) == MAX_COUNT == 8192
    assert "tf_rt_extrema.cpp" in compilers.RUNTIME_SOURCES     # (the code objects: tests/test_observer_objects.py)
    assert extrema.ExtremaSet.kind == "extrema"
    with pytest.raises(ValueError, match="kind of observer"):
        compilers.build_observer_code_object(_model("M2_diff"), "", "extremum")
    names = _capi.Library(compilers.build_runtime_library()).kernel_names()
    at = names.index("tfk_spectrum_final")
    assert names[at + 1:] == ["tfk_extrema_count", "tfk_extrema_write"] and len(names) <= 64


def test_extrema_is_a_kind_of_observer_code_object_and_does_not_spill():
    model = _model("M2_diff")
    block, _ = codegen.lower_extrema(model, [probes.discretise(model, "U"), probes.discretise(model, "k * dxxU")])
    hsaco = compilers.build_observer_code_object(model, block, "extrema")
    usage = compilers.resource_usage(hsaco)
    for kernel in ("tfk_extrema_count", "tfk_extrema_write"):
        assert usage[kernel]["ScratchSize"] == 0 and usage[kernel]["VGPRs"] > 0, (kernel, usage[kernel])


# ---- validation --------------------------------------------------------------------------------
def _sim(name="M2_diff", N=50):
    model = _model(name)
    fields = corpus.synthetic_fields(name, N)
    return Simulation(model, fields, corpus.synthetic_pars(name, N, True), dt=1e-3, time_stepping=False)


@pytest.mark.parametrize("kwargs,match", [
    (dict(kind="maximum"), "kind"),
    (dict(kind=0), "kind"),
    (dict(every=0), "every"),
    (dict(every=1.5), "every"),
    (dict(every=True), "every"),
    (dict(max_count=0), "max_count"),
    (dict(max_count=8193), "max_count"),
    (dict(max_count=2.0), "max_count"),
    (dict(max_count=True), "max_count"),
    (dict(capacity=0), "capacity"),
    (dict(capacity=1.5), "capacity"),
    (dict(threshold=np.nan), "threshold"),
    (dict(threshold=np.inf), "threshold"),
    (dict(threshold="1"), "threshold"),
])
def test_validation_errors(kwargs, match):
    with pytest.raises(ValueError, match=match) as err:
        _sim().add_extrema("c", "U", **kwargs)
    assert "extrema" in str(err.value)


def test_a_grid_of_two_nodes_is_refused_and_the_limits_are_accepted():
    es = extrema.ExtremaSet(_model("M2_diff"), 2)
    with pytest.raises(ValueError, match="N >= 3") as err:
        es.add("c", "U")
    assert "extrema" in str(err.value)
    es = extrema.ExtremaSet(_model("M2_diff"), 3)
    es.add("a", "U", max_count=1, capacity=1, threshold=0)
    es.add("b", "U", max_count=np.int32(8192), every=np.int64(2), threshold=np.float32(0.5), kind="min")
    assert es._items[0].threshold == 0.0 and es._items[0].device_threshold() == 0.0
    es.add("c", "U")
    es.add("d", "U", kind="min")
    assert es._items[2].device_threshold() == -np.inf and es._items[3].device_threshold() == np.inf


@pytest.mark.parametrize("expr", ["U *", "foo * U", "bar(U)", "dxk", 3])
def test_badly_formed_or_unknown_symbol(expr):
    with pytest.raises(ValueError, match="badly formated"):
        _sim().add_extrema("c", expr)


def test_heaviside_and_wide_stencils_are_refused():
    with pytest.raises(UnsupportedExpression, match="Heaviside"):
        _sim().add_extrema("c", "Heaviside(U - 1) * U")
    with pytest.raises(UnsupportedExpression, match="window"):
        _sim().add_extrema("c", "dxxxxU")


def test_duplicate_names_removal_and_the_limit():
    es = extrema.ExtremaSet(_model("M2_diff"), 50)
    es.add("a", "U", every=3)
    with pytest.raises(ValueError, match="named 'a' exists already") as err:
        es.add("a", "dxU")
    assert "extrema" in str(err.value)
    es.add("b", "dxU", kind="min")
    assert es.names == ["a", "b"]
    es.remove("a")
    assert es.names == ["b"]
    with pytest.raises(KeyError):
        es.remove("a")
    with pytest.raises(KeyError):
        _sim().remove_extrema("nope")
    t, n, g, x, v = es.series(per_system=False)["b"]
    assert t.shape == (0,) and n.shape == (0,) and g.shape == x.shape == v.shape == (0, 256)
    assert n.dtype == g.dtype == np.int64 and x.dtype == v.dtype == np.float64
    assert _sim().extrema == {}
    for i in range(MAX_EXTREMA - 1):
        es.add("s%d" % i, "U")
    assert len(es.names) == MAX_EXTREMA == 64
    with pytest.raises(ValueError, match="at most 64 extrema") as err:
        es.add("one more", "U")


# ---- the host side of a set ----------------------------------------------------------------------
class _FakeStepper:
    class compiled:
        pars = ["k"]
    solver = None

    def bind(self, fields, pars):
        pass

    def acquire(self, fields):
        return 0


def test_an_observer_that_cannot_run_is_not_kept(monkeypatch):
    def fail(self, solver):
        raise UnsupportedExpression("the extrema kernels need more registers than a wavefront has")
    import triflow_amd.simulation as simulation
    monkeypatch.setattr(simulation, "stepper_for", lambda *a, **k: _FakeStepper())
    sim = _sim()
    es = sim._extrema = extrema.ExtremaSet(sim.model, 50)
    es.add("kept", "U", max_count=2)
    kept = es._items[0]
    kept.last = kept.origin = sim.i
    kept.x = np.linspace(0, 1, 50)[None, :]
    kept.t, kept.blocks = [0.0], [np.array([[[1.0, 7.0, 0.0, 1.0, 0.0, -1.0, -1.0, -1.0, -1.0]]])]
    monkeypatch.setattr(extrema.ExtremaSet, "_bind", fail)
    with pytest.raises(UnsupportedExpression):
        sim.add_extrema("c", "U")
    assert list(sim.extrema) == ["kept"] and sim._extrema.names == ["kept"]
    t, n, g, x, v = sim.extrema["kept"]
    assert np.array_equal(t, [0.0]) and np.array_equal(n, [1]) and np.array_equal(g, [[7, -1]])
    assert sim.probes == {} and sim.recorders == {} and sim.statistics == {} and sim.spectra == {}
    sim.remove_extrema("kept")
    with pytest.raises(UnsupportedExpression):
        sim.add_extrema("c", "U")
    assert sim.extrema == {} and sim._extrema.names == []


class _Handle:
    """Stands in for _capi.DeviceExtrema: a row holds the number of the record as its count and one entry
    at that node; the calls are kept."""

    def __init__(self, solver, max_count):
        self.solver, self.calls, self.rows, self.max_count = solver, [], {}, max_count

    def set_x(self, x):
        pass

    def record(self, k, slot):
        self.calls.append(("record", k))
        self.rows.setdefault(k, []).append(float(len(self.calls)))

    def fetch(self, k):
        self.calls.append(("fetch", k))
        rows = self.rows.pop(k, [])
        out = np.zeros((len(rows), self.solver.nsys, 1 + 4 * self.max_count[k]))
        for i, c in enumerate(rows):
            out[i, :, 0] = 1.0
            out[i, :, 1:5] = (c, 1.0, 2.0, 1.0)
        return out

    def close(self):
        pass


class _Solver:
    nsys, N = 1, 50

    class model:
        spec = dict(uses_x=0)


def _fake_set():
    es = extrema.ExtremaSet(_model("M2_diff"), 50)
    bounds = {}

    def bind(solver):
        if solver.N != es.N:
            return extrema.ExtremaSet._bind(es, solver)
        if id(solver) not in bounds:
            bounds[id(solver)] = extrema._Bound(_Handle(solver, [r.max_count for r in es._items]), dict(host_consts=[]))
        return bounds[id(solver)]
    es._bind = bind
    return es, bounds


def test_only_observers_that_are_due_are_launched_and_a_change_of_solver_loses_no_row():
    es, bounds = _fake_set()
    x = np.linspace(0, 2, 50)
    first, second = _Solver(), _Solver()
    es.add("every1", "U", max_count=4)
    es.add("every3", "U", every=3, max_count=2, kind="min")
    dues = []
    for key in range(4, 11):
        dues.append(es.due(key))
        solver = first if key < 8 else second
        es.record(solver, 0, 0.1 * key, key, x, [[1.0]])
        es.record(solver, 0, 0.1 * key, key, x, [[1.0]])   # (the same state again: no second row)
    assert dues == [[0, 1], [0], [0], [0, 1], [0], [0], [0, 1]]
    s = es.series(per_system=False)
    t1, n1, g1, x1, v1 = s["every1"]
    t3, n3, g3, x3, v3 = s["every3"]
    assert g1.shape == (7, 4) and g3.shape == (3, 2) and (n1 == 1).all()
    assert np.allclose(t1, 0.1 * np.arange(4, 11)) and np.allclose(t3, [0.4, 0.7, 1.0])
    assert list(g1[:, 0]) == [1, 3, 4, 5, 1, 2, 3] and (g1[:, 1:] == -1).all()      # in record order
    assert list(g3[:, 0]) == [2, 6, 4]
    assert np.array_equal(x1[:, 0], x[g1[:, 0]]) and (v1[:, 0] == 2.0).all()         # a symmetric triple: the node
    assert np.isnan(x1[:, 1:]).all() and np.isnan(v1[:, 1:]).all()

    class Other(_Solver):
        N = 60
    with pytest.raises(ValueError, match="laid out for 50 nodes") as err:
        es.record(Other(), 0, 1.1, 11, np.linspace(0, 1, 60), [[1.0]])
    assert "extrema" in str(err.value)


def test_ensemble_series_keep_the_axis_of_the_systems():
    es, _ = _fake_set()

    class Three(_Solver):
        nsys = 3
    es.add("m", "U", max_count=5, refine=False)
    xs = np.array([np.linspace(0, 1 + e, 50) for e in range(3)])
    es.record(Three(), 0, 0.0, 0, xs, [[1.0]] * 3)
    t, n, g, x, v = es.series()["m"]
    assert n.shape == (1, 3) and g.shape == x.shape == v.shape == (1, 3, 5)
    assert np.array_equal(x[0, :, 0], xs[:, 1]) and (v[0, :, 0] == 2.0).all()


# ---- the refinement ------------------------------------------------------------------------------
def test_a_sampled_parabola_is_recovered_and_refine_false_returns_the_nodes():
    x = np.linspace(0.0, 2.0, 41)
    dx = (x[-1] - x[0]) / 40
    for x0, top, curv in ((0.7031, 1.5, -2.0), (1.21, -0.25, 3.0), (1.0, 2.0, -0.5)):
        v = top + curv * (x - x0) ** 2
        kind = "max" if curv < 0 else "min"
        g, tri = cases.referee(v, kind, False)
        assert g.size == 1 and abs(x[g[0]] - x0) <= dx / 2
        raw = np.zeros((1, 1, 1 + 4 * 3))
        raw[0, 0, :5] = (1.0, g[0], *tri[0])
        n, gg, xr, vr = extrema.ExtremaSet.rows_of(raw, x[None, :], True)
        assert n[0, 0] == 1 and list(gg[0, 0]) == [g[0], -1, -1]
        # the parabola through three samples of a parabola is that parabola: the vertex to rounding (a few
        # units of the last place of the values and of x)
        assert abs(xr[0, 0, 0] - x0) <= 64 * np.finfo(float).eps * max(abs(top / curv), 1.0)
        assert abs(vr[0, 0, 0] - top) <= 16 * np.finfo(float).eps * max(abs(top), 1.0)
        assert np.isnan(xr[0, 0, 1:]).all() and np.isnan(vr[0, 0, 1:]).all()
        rx, rv = cases.refined(x, g, tri)
        assert xr[0, 0, 0] == rx[0] and vr[0, 0, 0] == rv[0]                      # the issue's order of operations
        n, gg, xn, vn = extrema.ExtremaSet.rows_of(raw, x[None, :], False)
        assert xn[0, 0, 0] == x[g[0]] and vn[0, 0, 0] == v[g[0]]
        assert np.isnan(xn[0, 0, 1:]).all() and np.isnan(vn[0, 0, 1:]).all()
