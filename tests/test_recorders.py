"""Device recorders on the CPU: lowering, per-node values, columns and pools through the host harness
(tests/record_host: the generated record block and csrc/tf_record.h compiled with g++), validation,
the model left untouched, and the container round trip of a series."""
import math
import os

import numpy as np
import pytest
from sympy import lambdify

from oracle import corpus
from oracle import numpy_path as ora
from tests.record_host import build_record_host as host
from triflow_amd import Model, codegen, probes, recorders
from triflow_amd.codegen import UnsupportedExpression
from triflow_amd.container import retrieve_container, write_series
from triflow_amd.simulation import Simulation


def _model(name):
    return Model(*corpus.model_args(name), hold_compilation=True)


def numpy_nodes(model, exprs, inputs):
    """The per-node values NumPy computes: the lambdified discretised expressions with the
    reference's module dictionary, on the ghost-padded views of the reference."""
    disc = [probes.discretise(model, e) for e in exprs]
    f = lambdify(model._symbolic_args, disc, modules=ora._lambdify_modules())
    env, N, _, _ = ora.stencil_views(model, *inputs)
    with np.errstate(all="ignore"):
        vals = f(*[env[k] for k in model._args])
    return np.array([np.broadcast_to(np.asarray(v, dtype=float), (N,)) for v in vals])


def bins(values, nodes):
    start, stop, step = nodes.indices(values.size)
    return [values[g:min(g + step, stop)] for g in range(start, stop, step)]


def pooled(values, nodes, pool):
    """The columns NumPy gives ("mean": the exactly rounded sum over the count)."""
    with np.errstate(all="ignore"):
        if pool == "sample":
            return np.array([b[0] for b in bins(values, nodes)])
        if pool in ("max", "min"):
            return np.array([getattr(np, pool)(b) for b in bins(values, nodes)])
        return np.array([math.fsum(b) / b.size if np.isfinite(b).all() else np.sum(b) / b.size
                         for b in bins(values, nodes)])


def mean_bound(values, nodes):
    """|got - fsum(bin) / count| <= 2**-52 * fsum(|bin|): recursive summation of count terms,
    (count - 1) u sum|f|, divided by count, plus the rounding of the division, u = 2**-53; holds for
    any fixed order of the sum."""
    return np.array([2.0 ** -52 * math.fsum(np.abs(b)) for b in bins(values, nodes)])


# the models and expressions of tests/test_probes.py::CASES
CASES = [
    ("M1_advdiff", ["dxxU", "k * dxU**2", "U * x", "U * k**3 + c**2 / k"]),
    ("M3_film", ["dxxxh", "upwind(c, q, 2)", "q / h**2 + We * h * dxxxxh", "dx(h * q) - T**2 * eps**3"]),
    ("M5_stiff", ["k2 * B**2 - k4 * C * D", "upwind(c, D, 1) + Dm * dxxE"]),
    ("helper", ["s * dxxU", "dxs * U + s**2"]),
    ("upwind2_par", ["upwind(c, U, 2)", "c * dxU + k * x"]),
]
GRIDS = [(37, True, 5), (37, False, 4), (1003, True, 31), (1003, False, 300), (1003, True, 1)]


def windows(N):
    """Every node; windows that start at node 0, end at N - 1, start inside a chunk, have a short last
    bin, one column, a step beyond the grid."""
    return [slice(None), slice(3, 1001, 7), slice(None, None, 64), slice(5, 6), slice(0, None, N + 5),
            slice(N - 1, None), slice(11, None, 10), slice(None, N - 2, 9), slice(2, None, 300)]


def _setup(name, exprs, N, periodic, P):
    model = _model(name)
    per_node = name == "upwind2_par"
    fields = corpus.synthetic_fields(name, N, periodic=periodic)
    pars = corpus.synthetic_pars(name, N, periodic, per_node=per_node)
    dep, helps, parnames = corpus.field_names(name)
    mask = sum(1 << k for k, p in enumerate(parnames) if np.ndim(pars[p]) > 0) if per_node else 0
    h = host.Harness(model, exprs, fields["x"], fields, pars, periodic, P, mask)
    inputs = [fields["x"]] + [fields[k] for k in dep + helps] + [pars[k] for k in parnames] + [periodic]
    return h, numpy_nodes(model, exprs, inputs)


@pytest.mark.parametrize("name,exprs", CASES)
@pytest.mark.parametrize("N,periodic,P", GRIDS)
def test_nodes_and_sample_columns_bit_identical_to_numpy(name, exprs, N, periodic, P):
    h, ref = _setup(name, exprs, N, periodic, P)
    for k, e in enumerate(exprs):
        for nodes in windows(N):
            if nodes.indices(N)[1] <= nodes.indices(N)[0]:
                continue
            got = h.row(k, "sample", nodes)
            want = ref[k][nodes]
            assert got.shape == want.shape, (e, nodes)
            assert np.array_equal(got, want), (e, nodes, np.abs(got - want).max())


@pytest.mark.parametrize("name,exprs", CASES[:2])
@pytest.mark.parametrize("N,periodic,P", GRIDS)
def test_pooled_columns(name, exprs, N, periodic, P):
    h, ref = _setup(name, exprs, N, periodic, P)
    for k, e in enumerate(exprs):
        for nodes in windows(N):
            if nodes.indices(N)[1] <= nodes.indices(N)[0]:
                continue
            for pool in ("max", "min"):
                assert np.array_equal(h.row(k, pool, nodes), pooled(ref[k], nodes, pool)), (e, nodes, pool)
            got = h.row(k, "mean", nodes)
            err = np.abs(got - pooled(ref[k], nodes, "mean"))
            print(e, nodes, "mean: worst error / bound", np.max(err / np.maximum(mean_bound(ref[k], nodes), 1e-300)))
            assert (err <= mean_bound(ref[k], nodes)).all(), (e, nodes)


def _plain_harness(values, periodic, P):
    model = _model("M1_advdiff")
    N = values.size
    x = np.linspace(0.0, 3.0, N, endpoint=not periodic)
    return host.Harness(model, ["U"], x, dict(x=x, U=values), dict(k=.1, c=.2), periodic, P)


@pytest.mark.parametrize("N,P", [(37, 5), (1003, 31), (70001, 9000)])
@pytest.mark.parametrize("periodic", [True, False])
def test_pools_of_rough_data(N, P, periodic):
    rng = np.random.default_rng(N)
    f = rng.standard_normal(N) * np.exp(rng.uniform(-3, 3, N))
    h = _plain_harness(f, periodic, P)
    for nodes in (slice(None, None, 64), slice(3, N - 2, 7), slice(1, None, 1000), slice(None, None, 5000)):
        for pool in ("sample", "max", "min"):
            assert np.array_equal(h.row(0, pool, nodes), pooled(f, nodes, pool)), (nodes, pool)
        err = np.abs(h.row(0, "mean", nodes) - pooled(f, nodes, "mean"))
        assert (err <= mean_bound(f, nodes)).all(), nodes


def test_nan_and_inf_follow_numpy():
    N = 1003
    f = np.linspace(-1, 1, N)
    f[[250, 700, 701]] = np.nan
    f[[10, 400]] = np.inf
    f[[11, 900]] = -np.inf
    f[[64, 65, 66, 67]] = [np.inf, np.nan, -np.inf, 1.0]
    h = _plain_harness(f, True, 31)
    for nodes in (slice(None, None, 64), slice(None, None, 4), slice(2, 1000, 13), slice(None)):
        for pool in ("sample", "max", "min"):
            with np.errstate(invalid="ignore"):
                want = pooled(f, nodes, pool)
            got = h.row(0, pool, nodes)
            assert np.array_equal(got, want, equal_nan=True), (nodes, pool)
        got = h.row(0, "mean", nodes)
        for g, b in zip(got, bins(f, nodes)):
            if np.isfinite(b).all():
                assert abs(g - math.fsum(b) / b.size) <= 2.0 ** -52 * math.fsum(np.abs(b))
            else:
                with np.errstate(invalid="ignore"):
                    want = np.sum(b) / b.size            # nan, or the infinity of the bin
                assert (np.isnan(g) and np.isnan(want)) or g == want


# ---- lowering ----------------------------------------------------------------------------------
def test_record_block_and_spec():
    model = _model("M3_film")
    disc = [probes.discretise(model, e) for e in ("h", "dxh * k**3", "x * q")]
    block, spec = codegen.lower_records(model, disc)
    assert "#define TF_NREC 3" in block and "#define TF_REC_USES_X 1" in block
    assert "case 2: return" in block and "tf_eval_record(int k," in block
    assert "k ** 3" in spec["host_consts"] and spec["nrec"] == 3
    pblock, pspec = codegen.lower_probes(model, disc, ["sum"] * 3)
    assert pspec["host_consts"] == spec["host_consts"] and pspec["uses_x"] == spec["uses_x"]
    for k in range(3):          # the same C expressions, from the same emitter
        expr = [ln for ln in pblock.splitlines() if ln.startswith("    P[%d] = " % k)][0][len("    P[0] = "):]
        assert "    case %d: return %s" % (k, expr) in block


def test_the_record_kernel_follows_the_table():
    import re
    from triflow_amd import compilers
    with open(compilers.CSRC + "/tf_args.h") as f:
        text = f.read()
    assert re.search(r'TF_KERNEL_NAMES_RECORD \{ "tfk_record" \}', text)
    assert re.search(r"TFK_PROBE_FINAL,\s*TFK_RECORD, TFK_COUNT", text)
    assert "tf_rt_record.cpp" in compilers.RUNTIME_SOURCES      # (the code objects: tests/test_observer_objects.py)


# ---- validation --------------------------------------------------------------------------------
def _sim(name="M2_diff", N=50):
    model = _model(name)
    fields = corpus.synthetic_fields(name, N)
    return Simulation(model, fields, corpus.synthetic_pars(name, N, True), dt=1e-3, time_stepping=False)


@pytest.mark.parametrize("kwargs,match", [
    (dict(pool="median"), "pool"),
    (dict(every=0), "every"),
    (dict(every=1.5), "every"),
    (dict(nodes=slice(None, None, -1)), "step"),
    (dict(nodes=slice(None, None, 0)), "nodes"),
    (dict(nodes=5), "slice"),
    (dict(nodes=[1, 2]), "slice"),
    (dict(nodes=slice(10, 10)), "no node"),
    (dict(nodes=slice(60, None)), "no node"),
    (dict(capacity=1), "capacity"),
])
def test_validation_errors(kwargs, match):
    with pytest.raises(ValueError, match=match):
        _sim().add_recorder("r", "U", **kwargs)


@pytest.mark.parametrize("expr", ["U *", "foo * U", "bar(U)", "dxk"])
def test_badly_formed_or_unknown_symbol(expr):
    with pytest.raises(ValueError, match="badly formated"):
        _sim().add_recorder("r", expr)


def test_wider_stencil_than_the_window_names_the_limit():
    with pytest.raises(UnsupportedExpression, match=r"half width 1\b"):
        _sim("M2_diff").add_recorder("r", "dxxxU", pool="max")


def test_duplicate_names_and_removal():
    rs = recorders.RecorderSet(_model("M2_diff"), 50)
    rs.add("a", "U", every=3, nodes=slice(None, None, 4), pool="mean")
    with pytest.raises(ValueError, match="exists already"):
        rs.add("a", "dxU")
    rs.add("b", "dxU")
    assert rs.names == ["a", "b"]
    rs.remove("a")
    assert rs.names == ["b"]
    with pytest.raises(KeyError):
        rs.remove("a")
    with pytest.raises(KeyError):
        _sim().remove_recorder("nope")
    t, x, v = rs.series(per_system=False)["b"]
    assert t.shape == (0,) and x.shape == (50,) and v.shape == (0, 50)
    assert _sim().recorders == {}


def test_default_ring_is_sized_in_bytes_and_refuses_a_row_that_does_not_fit():
    rs = recorders.RecorderSet(_model("M2_diff"), 10 ** 7)
    rs.add("wide", "U")
    rs.add("thin", "U", nodes=slice(None, None, 10 ** 4))
    rs.add("fixed", "U", capacity=5)
    wide, thin, fixed = rs._items
    with pytest.raises(ValueError, match="does not fit"):
        wide.rows_of_ring(1)                              # 80 MB a row
    assert thin.rows_of_ring(1) == recorders.MAX_RING_ROWS
    assert thin.rows_of_ring(64) * 8 * 64 * thin.ncols <= recorders.DEFAULT_RING_BYTES
    assert fixed.rows_of_ring(1) == 4                     # (two halves of two rows)
    rs2 = recorders.RecorderSet(_model("M2_diff"), 10 ** 6)
    rs2.add("all", "U")
    assert rs2._items[0].rows_of_ring(1) == 4 and rs2._items[0].rows_of_ring(1) * 8e6 <= recorders.DEFAULT_RING_BYTES


def test_model_untouched():
    model = _model("M2_diff")
    bounds, window = model._bounds, model._window_range
    footprint = {k: set(v) for k, v in model._symb_vars_with_spatial_diff_order.items()}
    src, spec = codegen.lower_model(model)
    tag = codegen.source_hash(src)
    rs = recorders.RecorderSet(model, 100)
    rs.add("a", "dxU**2 + k**3", nodes=slice(None, None, 8), pool="mean")
    rs.add("b", "U * x", every=5)
    with pytest.raises(UnsupportedExpression):
        rs.add("c", "dxxxxU")
    assert model._bounds == bounds and model._window_range == window
    assert {k: set(v) for k, v in model._symb_vars_with_spatial_diff_order.items()} == footprint
    src2, spec2 = codegen.lower_model(model)
    assert src2 == src and codegen.source_hash(src2) == tag and spec2 == spec
    assert rs.names == ["a", "b"]


class _FakeStepper:
    class compiled:
        pars = ["k"]
    solver = None

    def bind(self, fields, pars):
        pass

    def acquire(self, fields):
        return 0


def test_recorder_that_cannot_run_is_not_kept(monkeypatch):
    def fail(self, solver):
        raise UnsupportedExpression("the record kernels need more registers than a wavefront has")
    monkeypatch.setattr(recorders.RecorderSet, "_bind", fail)
    import triflow_amd.simulation as simulation
    monkeypatch.setattr(simulation, "stepper_for", lambda *a, **k: _FakeStepper())
    sim = _sim()
    with pytest.raises(UnsupportedExpression):
        sim.add_recorder("r", "U", pool="max")
    assert sim.recorders == {} and sim._recorders.names == []


def test_only_recorders_that_are_due_are_launched():
    class Handle:
        solver = object()

        def __init__(self):
            self.calls, self.fetched = [], {}

        def record(self, k, slot):
            self.calls.append(k)

        def set_x(self, x):
            pass

        def fetch(self, k):
            n, self.fetched[k] = self.calls.count(k) - self.fetched.get(k, 0), self.calls.count(k)
            return np.zeros((n, 1, 1))

        def close(self):
            pass

    class Solver:
        nsys, N = 1, 50
        class model:
            spec = dict(uses_x=0)

    rs = recorders.RecorderSet(_model("M2_diff"), 50)
    handle = Handle()
    bound = recorders._Bound(handle, dict(host_consts=[]))
    rs._bind = lambda solver: bound
    x = np.linspace(0, 1, 50)
    rs.add("every1", "U", nodes=slice(7, 8))
    rs.record(Solver, 0, 0.0, 4, x, [[1.0]])
    rs.add("every3", "U", every=3, nodes=slice(7, 8))
    rs.record(Solver, 0, 0.0, 4, x, [[1.0]])              # (the t0 row of the new one only)
    assert handle.calls == [0, 1]
    for key in range(5, 12):
        rs.record(Solver, 0, 0.1 * key, key, x, [[1.0]])
    assert handle.calls == [0, 1] + [0, 0, 0, 1, 0, 0, 0, 1, 0]
    s = rs.series(per_system=False)
    assert len(s["every1"][0]) == 8 and np.allclose(s["every3"][0], [0.0, 0.7, 1.0])
    assert np.array_equal(s["every1"][1], x[7:8])


# ---- the container of a series ------------------------------------------------------------------
def test_write_series_round_trip(tmp_path):
    from scipy.io import netcdf_file
    rng = np.random.default_rng(3)
    t = np.arange(7) * 0.01
    x = np.linspace(0, 5, 33)
    h, q = rng.standard_normal((7, 33)), rng.standard_normal((7, 33))
    meta = dict(Re=15.0, periodic=True, n=3, name="film")
    path = write_series(str(tmp_path / "series"), t, x, dict(h=h, q=q), meta)
    got = retrieve_container(path)
    assert sorted(got.data) == ["h", "q", "t", "x"]
    assert np.array_equal(got.data["t"], t) and np.array_equal(got.data["x"], x)
    assert np.array_equal(got.data["h"], h) and np.array_equal(got.data["q"], q)
    assert got.metadata == meta
    with netcdf_file(os.path.join(path, "data.nc"), "r", mmap=False) as nc:
        assert dict(nc.dimensions) == {"t": 7, "x": 33}
        assert nc.variables["h"].dimensions == ("t", "x")
        assert nc.Re == 15.0
    with pytest.raises(ValueError):
        write_series(str(tmp_path / "bad"), t, x, dict(h=h[:, :5]))
