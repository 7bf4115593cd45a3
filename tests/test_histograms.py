"""Device histograms on the CPU: the referee (tests/hist_cases.py) against both forms of np.histogram, the
classification, the window and the walk through the host harness (tests/hist_host: the generated histogram
block and csrc/tf_histogram.h compiled with g++) against the referee -- exactly, every node --, lowering,
the "histogram" kind of code object and what it leaves alone, validation and the host side of a set."""
import re
import subprocess

import numpy as np
import pytest

from oracle import corpus
from tests import hist_cases as cases
from tests.hist_host import build_hist_host as host
from tests.test_statistics import numpy_nodes
from triflow_amd import Model, _capi, codegen, compilers, histograms, probes
from triflow_amd.codegen import UnsupportedExpression
from triflow_amd.histograms import MAX_BINS, MAX_HISTOGRAMS
from triflow_amd.simulation import Simulation

_MODELS = {}


def _model(name):
    if name not in _MODELS:
        _MODELS[name] = Model(*corpus.model_args(name), hold_compilation=True)
    return _MODELS[name]


# ---- the referee ---------------------------------------------------------------------------------
def test_the_referee_is_np_histogram():
    """Both forms, on values placed on every edge and one ulp to either side, NaN, the infinities and the
    zeros, a constant field and a field with every node outside."""
    rs = np.random.RandomState(3)
    sets = cases.edge_sets()
    for _ in range(40):
        n = int(rs.randint(1, MAX_BINS + 1))
        lo = float(rs.uniform(-3, 3))
        hi = lo + float(10.0 ** rs.uniform(-6, 3))
        sets.append((np.linspace(lo, hi, n + 1), (n, lo, hi)))
    for edges, uniform in sets:
        adv = cases.adversarial(edges)
        for v in (adv, cases.cycled(adv, 3 * adv.size + 1), np.full(100, edges[0]), np.full(100, edges[-1]),
                  np.full(7, edges[-1] + 1.0), np.full(7, edges[0] - 1.0),
                  np.concatenate([np.full(5, -np.inf), np.full(3, np.nan)]),
                  rs.uniform(edges[0], edges[-1], 500)):
            counts = cases.check_against_numpy(v, edges, uniform)
            c2, outside = cases.referee(v, edges)
            assert np.array_equal(counts, c2) and counts.sum() + outside.sum() == np.size(v)
    # what the rule says in so many words
    c, o = cases.referee([0.0, -0.0, 1.0, 2.0, 3.0, np.nextafter(3.0, 4.0), -1e-300, np.nan, np.inf, -np.inf],
                         [0.0, 1.0, 2.0, 3.0])
    assert list(c) == [2, 1, 2] and list(o) == [2, 2, 1]


# ---- the walk through the host harness -------------------------------------------------------------
# (model, periodic, expressions, the field that expression 0 is, per-node parameters)
CASES = [("M3_film", True, ["h", "We * h * dxxxh", "x"], "h", False),
         ("M1_advdiff", False, ["U", "c * dxU**2"], "U", False),
         ("upwind2_par", True, ["U", "c * dxU"], "U", True)]
# chunks of 3 | 50 | 9 9 9 9 9 8 | 5 5 4 ... (257 chunks of 4 / 5 nodes: two workgroups, the second with one
# chunk) | 17 x 7, 16 x 253 (260 chunks: three segments of 8, the last of one node) | 5 x 76, 4 x 524 (600
# chunks: three workgroups)
GRIDS = [(3, 1), (50, 1), (53, 6), (1030, 257), (4167, 260), (2476, 600)]
WINDOWS = [slice(None), slice(5, -3, 7), slice(2, None, 1), slice(None, None, 8)]
_HARNESS = {}


def _harness(name, periodic, exprs, per_node, N, P):
    key = (name, N, P)
    if key not in _HARNESS:
        model = _model(name)
        pars = corpus.synthetic_pars(name, N, periodic, per_node=per_node)
        fields = corpus.synthetic_fields(name, N, seed=1, periodic=periodic)
        parnames = corpus.field_names(name)[2]
        mask = sum(1 << k for k, p in enumerate(parnames) if np.ndim(pars[p]) > 0) if per_node else 0
        _HARNESS[key] = (host.Harness(model, exprs, fields["x"], pars, periodic, P, mask), fields, pars)
    return _HARNESS[key]


def _check(h, which, edges, fields, v, nodes=slice(None), label=""):
    counts, outside = h.run(which, edges, fields, nodes)
    rc, ro = cases.referee(np.asarray(v)[nodes], edges)
    assert np.array_equal(counts, rc), (label, counts, rc)
    assert np.array_equal(outside, ro), (label, outside, ro)
    assert counts.dtype == outside.dtype == np.int64
    assert counts.sum() + outside.sum() == len(range(*nodes.indices(len(v)))), label
    return counts, outside


@pytest.mark.parametrize("name,periodic,exprs,var,per_node", CASES, ids=[c[0] for c in CASES])
@pytest.mark.parametrize("N,P", GRIDS)
def test_walk_against_the_referee(name, periodic, exprs, var, per_node, N, P):
    """Crafted fields through expression 0 (the field itself): every edge and its neighbours, NaN, the
    infinities and the zeros, a constant field, every node outside; then every expression of the block on
    the synthetic state, a derivative among them, so that the node window crosses the chunk borders."""
    h, fields, pars = _harness(name, periodic, exprs, per_node, N, P)
    for edges, _ in cases.edge_sets():
        adv = cases.adversarial(edges)
        crafted = dict(edges=cases.cycled(adv, N), constant=np.full(N, edges[0]), top=np.full(N, edges[-1]),
                       above=np.full(N, np.nextafter(edges[-1], np.inf)), below=np.full(N, -np.inf))
        for label, v in crafted.items():
            for nodes in WINDOWS if label == "edges" else WINDOWS[:2]:
                if len(range(*nodes.indices(N))) == 0:
                    continue
                c, o = _check(h, 0, edges, dict(fields, **{var: v}), v, nodes, (label, edges.size, N, P, nodes))
                if label == "top":
                    assert c[-1] == c.sum() + o.sum()                  # v == edges[-1]: the last bin
                if label == "constant":
                    assert c[0] == c.sum() + o.sum()
                if label in ("above", "below"):
                    assert c.sum() == 0 and o[2] == 0
    nodes_np = numpy_nodes(_model(name), exprs, fields, pars)
    for which, e in enumerate(exprs):
        v = nodes_np[which]
        lo, hi = float(np.min(v)), float(np.max(v))
        q = np.quantile(v, [0.1, 0.9])
        for edges in (np.linspace(lo, hi, 65), np.linspace(q[0], q[1], 257), np.unique(v)[:MAX_BINS + 1],
                      np.array([lo, hi])):
            if edges.size < 2:
                continue
            for nodes in WINDOWS[:2]:
                if len(range(*nodes.indices(N))):
                    _check(h, which, edges, fields, v, nodes, (e, edges.size, N, P, nodes))
    assert h.sets == -(-P // 256) * -(-(-(-N // P)) // 8)


def test_an_empty_window_and_windows_at_the_ends():
    name, periodic, exprs, var, per_node = CASES[0]
    N, P = 1030, 257
    h, fields, _ = _harness(name, periodic, exprs, per_node, N, P)
    edges = np.linspace(0.0, 3.0, 65)
    v = cases.cycled(cases.adversarial(edges), N)
    f = dict(fields, h=v)
    for window in ((7, 7, 1), (1030, 1030, 3), (500, 400, 2)):
        counts, outside = h.run(0, edges, f, window=window)
        assert counts.sum() == 0 and outside.sum() == 0, window
    for nodes in (slice(0, 1), slice(N - 1, N), slice(N - 1, None, 5), slice(4, 5), slice(0, N, N - 1)):
        _check(h, 0, edges, f, v, nodes, nodes)


def test_classification_alone():
    lib = _harness(*CASES[1][:3], False, 50, 1)[0].lib
    assert lib.hist_host_max_bins() == MAX_BINS == 256 and lib.hist_host_nhist() == 2
    for edges, _ in cases.edge_sets():
        nb = edges.size - 1
        for v in cases.adversarial(edges):
            c, o = cases.referee([v], edges)
            want = int(np.argmax(c)) if c.sum() else nb + int(np.argmax(o))
            assert host.classify(lib, v, edges) == want, (v, edges)
    e = np.array([0.0, 1.0])
    assert host.classify(lib, -0.0, e) == 0 and host.classify(lib, 1.0, e) == 0
    assert host.classify(lib, np.nextafter(0.0, -1.0), e) == 1 and host.classify(lib, np.nextafter(1.0, 2.0), e) == 2
    assert host.classify(lib, np.nan, e) == 3


# ---- lowering and the code objects -----------------------------------------------------------------
def test_histogram_block_and_spec():
    model = _model("M3_film")
    disc = [probes.discretise(model, e) for e in ("h", "dxh * k**3", "x * q")]
    block, spec = codegen.lower_histograms(model, disc)
    assert "#define TF_NHIST 3" in block and "#define TF_HIST_USES_X 1" in block and "#define TF_NHIST_HC 1" in block
    assert "tf_eval_hist(int k," in block and spec["nhist"] == 3
    rblock, rspec = codegen.lower_records(model, disc)
    assert rspec["host_consts"] == spec["host_consts"] and rspec["uses_x"] == spec["uses_x"]
    lines = [ln for ln in rblock.splitlines() if ln.startswith("    case ")]
    assert len(lines) == 3 and lines == [ln for ln in block.splitlines() if ln.startswith("    case ")]
    with pytest.raises(UnsupportedExpression, match="Heaviside"):
        codegen.lower_histograms(model, [probes.discretise(model, "Heaviside(h - 1)")])


def test_sets_that_differ_in_edges_window_or_every_share_a_block():
    a = histograms.HistogramSet(_model("M2_diff"), 50)
    a.add("p", "U", bins=64, range=(0.0, 3.0))
    a.add("q", "dxU", bins=[-1.0, 0.0, 0.5, 4.0])
    b = histograms.HistogramSet(_model("M2_diff"), 50)
    b.add("r", "U", bins=7, range=(-1.0, 1.0), every=7, nodes=slice(5, -3, 7))
    b.add("s", "dxU", bins=256, range=(0, 1), capacity=3, nodes=slice(None, None, 2))
    b.add("t", "U", bins=np.linspace(0, 1, 5))              # the same expression again: the same case
    assert len(b.expressions()) == 2
    assert a._lower(0)[0] == b._lower(0)[0]
    assert a._lower(0)[1] == b._lower(0)[1]


def _symbols(hsaco):
    return subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-readelf", "-s", hsaco], capture_output=True, text=True,
                          check=True).stdout


def test_histogram_is_a_kind_of_code_object_of_its_own_and_does_not_spill():
    """The "histogram" code object cross-compiles for gfx950 and holds the two kernels without scratch; the
    model's own code object and another observer's do not hold them (what else each holds:
    tests/test_observer_objects.py)."""
    model = _model("M2_diff")
    disc = [probes.discretise(model, "U"), probes.discretise(model, "k * dxxU")]
    block, _ = codegen.lower_histograms(model, disc)
    hsaco = compilers.build_observer_code_object(model, block, "histogram")
    usage = compilers.resource_usage(hsaco)
    syms = _symbols(hsaco)
    for kernel in ("tfk_hist_partial", "tfk_hist_final"):
        assert usage[kernel]["ScratchSize"] == 0 and usage[kernel]["VGPRs"] > 0, (kernel, usage[kernel])
        assert re.search(r"\b%s\b" % kernel, syms), kernel
    plain, _ = compilers.build_code_object(model)
    other = compilers.build_observer_code_object(model, codegen.lower_spectra(model, disc)[0], "spectrum")
    for path in (plain, other):
        assert "tfk_hist" not in _symbols(path), path
        assert not [k for k in compilers.resource_usage(path) if k.startswith("tfk_hist")], path
    assert "tf_rt_histogram.cpp" in compilers.RUNTIME_SOURCES
    assert histograms.HistogramSet.kind == "histogram"
    with pytest.raises(ValueError, match="kind of observer"):
        compilers.build_observer_code_object(model, "", "hist")


def test_the_kernel_table_is_what_it_was():
    names = _capi.Library(compilers.build_runtime_library()).kernel_names()
    assert len(names) == 52 and names[-2:] == ["tfk_extrema_count", "tfk_extrema_write"]
    assert names[44:] == ["tfk_probe_partial", "tfk_probe_final", "tfk_record", "tfk_stat", "tfk_spectrum_partial",
                          "tfk_spectrum_final", "tfk_extrema_count", "tfk_extrema_write"]
    assert not [n for n in names if "hist" in n]
    with open(compilers.CSRC + "/tf_args.h") as f:
        text = f.read()
    assert int(re.search(r"#define TF_HIST_MAX_BINS (\d+)", text).group(1)) == MAX_BINS
    assert "TFK_HIST" not in text


# ---- validation --------------------------------------------------------------------------------
def _sim(name="M2_diff", N=50):
    model = _model(name)
    fields = corpus.synthetic_fields(name, N)
    return Simulation(model, fields, corpus.synthetic_pars(name, N, True), dt=1e-3, time_stepping=False)


@pytest.mark.parametrize("kwargs,match", [
    (dict(bins=0, range=(0, 1)), "bins"),
    (dict(bins=257, range=(0, 1)), "bins"),
    (dict(bins=-3, range=(0, 1)), "bins"),
    (dict(bins=True, range=(0, 1)), "bins"),
    (dict(bins=None), "bins"),
    (dict(bins=2.5, range=(0, 1)), "edges"),
    (dict(bins=64), "no automatic range"),
    (dict(bins="auto"), "no automatic"),
    (dict(bins=64, range=(1.0, 1.0)), "lo < hi"),
    (dict(bins=64, range=(2.0, 1.0)), "lo < hi"),
    (dict(bins=64, range=(0.0, np.inf)), "finite"),
    (dict(bins=64, range=(np.nan, 1.0)), "finite"),
    (dict(bins=64, range=(0.0, 1.0, 2.0)), "pair"),
    (dict(bins=64, range=3.0), "pair"),
    (dict(bins=256, range=(1.0, np.nextafter(1.0, 2.0))), "too narrow"),
    (dict(bins=[0.0, 1.0], range=(0.0, 1.0)), "range"),
    (dict(bins=[1.0]), "edges"),
    (dict(bins=[]), "edges"),
    (dict(bins=np.linspace(0, 1, 258)), "edges"),
    (dict(bins=[[0.0, 1.0], [2.0, 3.0]]), "1-D"),
    (dict(bins=[0.0, 1.0, 1.0]), "strictly increasing"),
    (dict(bins=[0.0, 2.0, 1.0]), "strictly increasing"),
    (dict(bins=[0.0, np.nan, 1.0]), "finite"),
    (dict(bins=[0.0, 1.0, np.inf]), "finite"),
    (dict(bins=["a", "b"]), "edges"),
    (dict(bins=4, range=(0, 1), every=0), "every"),
    (dict(bins=4, range=(0, 1), every=1.5), "every"),
    (dict(bins=4, range=(0, 1), every=True), "every"),
    (dict(bins=4, range=(0, 1), capacity=0), "capacity"),
    (dict(bins=4, range=(0, 1), capacity=1.5), "capacity"),
    (dict(bins=4, range=(0, 1), nodes=5), "slice"),
    (dict(bins=4, range=(0, 1), nodes=[1, 2]), "slice"),
    (dict(bins=4, range=(0, 1), nodes=slice(None, None, -1)), "step"),
    (dict(bins=4, range=(0, 1), nodes=slice(None, None, 0)), "nodes"),
    (dict(bins=4, range=(0, 1), nodes=slice(40, 10)), "no node"),
    (dict(bins=4, range=(0, 1), nodes=slice(60, None)), "no node"),
    (dict(bins=4, range=(0, 1), nodes=slice(1.5, None)), "nodes"),
])
def test_validation_errors(kwargs, match):
    with pytest.raises(ValueError, match=match) as err:
        _sim().add_histogram("p", "U", **kwargs)
    assert "histogram" in str(err.value)


def test_the_limits_are_accepted_and_the_edges_are_linspace():
    hs = histograms.HistogramSet(_model("M2_diff"), 50)
    hs.add("a", "U", bins=1, range=(0, 1), capacity=1)
    hs.add("b", "U", bins=np.int32(256), range=(np.float32(0.5), 3), every=np.int64(2), nodes=slice(49, None))
    hs.add("c", "U", bins=np.linspace(-1, 1, 257))
    hs.add("d", "U", bins=(0.0, 5e-324))
    assert np.array_equal(hs._items[0].edges, [0.0, 1.0]) and hs._items[0].capacity == 1
    assert hs._items[1].edges.tobytes() == np.linspace(0.5, 3.0, 257).tobytes() and hs._items[1].window == (49, 50, 1)
    assert hs._items[2].nbins == 256 and hs._items[3].nbins == 1
    assert hs._items[0].edges.dtype == np.float64
    given = np.array([0.0, 1.0, 2.0])
    hs.add("e", "U", bins=given)
    given[1] = 5.0                                            # (the set keeps a copy)
    assert np.array_equal(hs._items[4].edges, [0.0, 1.0, 2.0])


@pytest.mark.parametrize("expr", ["U *", "foo * U", "bar(U)", "dxk", 3])
def test_badly_formed_or_unknown_symbol(expr):
    with pytest.raises(ValueError, match="badly formated"):
        _sim().add_histogram("p", expr, bins=4, range=(0, 1))


def test_heaviside_and_too_wide_stencils_are_refused():
    with pytest.raises(UnsupportedExpression, match="Heaviside"):
        _sim().add_histogram("p", "Heaviside(U - 1) * U", bins=4, range=(0, 1))
    with pytest.raises(UnsupportedExpression, match="offset"):
        _sim().add_histogram("p", "dxxxxU", bins=4, range=(0, 1))


def test_duplicate_names_removal_and_the_limit():
    hs = histograms.HistogramSet(_model("M2_diff"), 50)
    hs.add("a", "U", bins=5, range=(0, 1), every=3)
    with pytest.raises(ValueError, match="histogram named 'a' exists already"):
        hs.add("a", "dxU", bins=5, range=(0, 1))
    hs.add("b", "dxU", bins=[0.0, 0.5, 4.0])
    assert hs.names == ["a", "b"] and len(hs.expressions()) == 2
    hs.remove("a")
    assert hs.names == ["b"]
    with pytest.raises(KeyError):
        hs.remove("a")
    with pytest.raises(KeyError):
        _sim().remove_histogram("nope")
    t, edges, counts, outside = hs.series(per_system=False)["b"]
    assert t.shape == (0,) and np.array_equal(edges, [0.0, 0.5, 4.0])
    assert counts.shape == (0, 2) and outside.shape == (0, 3) and counts.dtype == outside.dtype == np.int64
    t, edges, counts, outside = hs.series()["b"]
    assert counts.shape == (0, 1, 2) and outside.shape == (0, 1, 3)
    assert _sim().histograms == {}
    for i in range(MAX_HISTOGRAMS - 1):
        hs.add("s%d" % i, "U", bins=1 + i, range=(0, 1))
    assert len(hs.names) == MAX_HISTOGRAMS == 64
    with pytest.raises(ValueError, match="at most 64 histograms") as err:
        hs.add("one more", "U", bins=4, range=(0, 1))
    assert "histogram" in str(err.value)


# ---- the host side of a set ----------------------------------------------------------------------
class _FakeStepper:
    class compiled:
        pars = ["k"]
    solver = None

    def bind(self, fields, pars):
        pass

    def acquire(self, fields):
        return 0


def test_histogram_that_cannot_run_is_not_kept(monkeypatch):
    def fail(self, solver):
        raise UnsupportedExpression("the histogram kernels need more registers than a wavefront has")
    import triflow_amd.simulation as simulation
    monkeypatch.setattr(simulation, "stepper_for", lambda *a, **k: _FakeStepper())
    sim = _sim()
    monkeypatch.setattr(histograms.HistogramSet, "_bind", fail)
    with pytest.raises(UnsupportedExpression):
        sim.add_histogram("p", "U", bins=4, range=(0, 1))
    assert sim.histograms == {} and sim._histograms.names == []
    assert sim.probes == {} and sim.extrema == {}


class _Handle:
    """Stands in for _capi.DeviceHistogram: a row holds the number of the record, the calls are kept."""

    def __init__(self, solver, nbins):
        self.solver, self.calls, self.rows, self.nbins = solver, [], {}, nbins

    def set_x(self, x):
        pass

    def record(self, k, slot):
        self.calls.append(("record", k))
        self.rows.setdefault(k, []).append(len(self.calls))

    def fetch(self, k):
        self.calls.append(("fetch", k))
        rows = self.rows.pop(k, [])
        return np.array(rows, dtype=np.int64).reshape(-1, 1, 1) * np.ones((1, self.solver.nsys, self.nbins[k] + 3),
                                                                         dtype=np.int64)

    def close(self):
        pass


class _Solver:
    nsys, N = 1, 50

    class model:
        spec = dict(uses_x=0)


def _fake_set():
    hs = histograms.HistogramSet(_model("M2_diff"), 50)
    bounds = {}

    def bind(solver):
        if solver.N != hs.N:
            return histograms.HistogramSet._bind(hs, solver)
        if id(solver) not in bounds:
            bounds[id(solver)] = histograms._Bound(_Handle(solver, [r.nbins for r in hs._items]), dict(host_consts=[]))
        return bounds[id(solver)]
    hs._bind = bind
    return hs, bounds


def test_only_histograms_that_are_due_are_launched():
    hs, bounds = _fake_set()
    x = np.linspace(0, 2, 50)
    solver = _Solver()
    hs.add("every1", "U", bins=3, range=(0, 1))
    assert hs.due(4) == [0]
    hs.record(solver, 0, 0.4, 4, x, [[1.0]])
    assert hs.due(4) == [] and hs.due(5) == [0]
    hs.add("every3", "U", bins=[0.0, 1.0], every=3)
    bounds.clear()                                         # (add closed the handles: a new one is bound)
    assert hs.due(4) == [1]
    hs.record(solver, 0, 0.4, 4, x, [[1.0]])               # (the first row of the new one only)
    handle = bounds[id(solver)].handle
    assert handle.calls == [("record", 1)]
    dues = []
    for key in range(5, 12):
        dues.append(hs.due(key))
        hs.record(solver, 0, 0.1 * key, key, x, [[1.0]])
        hs.record(solver, 0, 0.1 * key, key, x, [[1.0]])   # (the same state again: no second row)
    assert dues == [[0], [0], [0, 1], [0], [0], [0, 1], [0]]
    s = hs.series(per_system=False)
    t1, e1, c1, o1 = s["every1"]
    t3, e3, c3, o3 = s["every3"]
    assert c1.shape == (8, 3) and o1.shape == (8, 3) and c3.shape == (3, 1) and o3.shape == (3, 3)
    assert np.allclose(t1, [0.4] + [0.1 * k for k in range(5, 12)]) and np.allclose(t3, [0.4, 0.7, 1.0])
    assert np.array_equal(e1, np.linspace(0, 1, 4)) and np.array_equal(e3, [0.0, 1.0])
    assert np.array_equal(c3[:, 0], [1, 5, 9]) and np.array_equal(o3[:, 2], [1, 5, 9])   # in record order


def test_a_change_of_solver_loses_no_row_and_another_grid_is_refused():
    hs, bounds = _fake_set()
    x = np.linspace(0, 1, 50)
    first, second = _Solver(), _Solver()
    hs.add("m", "U", bins=2, range=(0, 1))
    for key in range(4):
        hs.record(first, 0, 0.1 * key, key, x, [[1.0]])
    for key in range(4, 7):
        hs.record(second, 0, 0.1 * key, key, x, [[1.0]])
    t, e, c, o = hs.series(per_system=False)["m"]
    assert c.shape == (7, 2) and np.array_equal(c[:, 0], [1, 2, 3, 4, 1, 2, 3])
    assert np.allclose(t, 0.1 * np.arange(7))

    class Other(_Solver):
        N = 60
    with pytest.raises(ValueError, match="laid out for 50 nodes") as err:
        hs.record(Other(), 0, 0.7, 7, np.linspace(0, 1, 60), [[1.0]])
    assert "histogram" in str(err.value)

    class Eight(_Solver):
        nsys = 8
    hs2, _ = _fake_set()
    hs2.add("m", "U", bins=5, range=(0, 1))
    hs2.record(Eight(), 0, 0.0, 0, np.tile(x, (8, 1)), [[1.0]] * 8)
    t, e, c, o = hs2.series()["m"]
    assert c.shape == (1, 8, 5) and o.shape == (1, 8, 3) and e.shape == (6,)


def test_the_emulation_back_end_has_no_histogram_kernels():
    """tests/emu links the weak definitions of the by-name seam: creating a set there is an error that says
    so, not a crash."""
    from functools import partial

    from tests.emu.build_emu import EmuBackend
    from triflow_amd.compilers import hip_compiler
    model = Model(*corpus.model_args("M2_diff"), compiler=partial(hip_compiler, backend=EmuBackend()))
    fields = corpus.synthetic_fields("M2_diff", 50)
    sim = Simulation(model, fields, corpus.synthetic_pars("M2_diff", 50, True), dt=1e-3, time_stepping=False)
    with pytest.raises(Exception, match="not supported by this back end"):
        sim.add_histogram("p", "U", bins=4, range=(0, 1))
    assert sim.histograms == {}
