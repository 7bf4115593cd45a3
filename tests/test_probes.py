"""Device probes on the CPU: lowering, per-node values and reductions through the host harness
(tests/probe_host: the generated probe block and csrc/tf_probe.h compiled with g++), validation,
and the model left untouched."""
import math
import re

import numpy as np
import pytest
from sympy import lambdify

from oracle import corpus
from oracle import numpy_path as ora
from tests.probe_host import build_probe_host as host
from triflow_amd import Model, codegen, probes
from triflow_amd.codegen import UnsupportedExpression
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


# (model, expressions): derivatives up to the window, upwind, a help function, a per-node parameter
# (upwind2_par with per-node c), x, a uniform pow
CASES = [
    ("M1_advdiff", ["dxxU", "k * dxU**2", "U * x", "U * k**3 + c**2 / k"]),
    ("M3_film", ["dxxxh", "upwind(c, q, 2)", "q / h**2 + We * h * dxxxxh", "dx(h * q) - T**2 * eps**3"]),
    ("M5_stiff", ["k2 * B**2 - k4 * C * D", "upwind(c, D, 1) + Dm * dxxE"]),
    ("helper", ["s * dxxU", "dxs * U + s**2"]),
    ("upwind2_par", ["upwind(c, U, 2)", "c * dxU + k * x"]),
]


@pytest.mark.parametrize("name,exprs", CASES)
@pytest.mark.parametrize("N,periodic,P", [(37, True, 5), (37, False, 4), (1003, True, 31), (1003, False, 300)])
def test_per_node_values_bit_identical_to_numpy(name, exprs, N, periodic, P):
    model = _model(name)
    per_node = name == "upwind2_par"
    fields = corpus.synthetic_fields(name, N, periodic=periodic)
    pars = corpus.synthetic_pars(name, N, periodic, per_node=per_node)
    dep, helps, parnames = corpus.field_names(name)
    mask = sum(1 << k for k, p in enumerate(parnames) if np.ndim(pars[p]) > 0) if per_node else 0
    nodes, _ = host.run(model, exprs, ["sum"] * len(exprs), fields["x"], fields, pars, periodic, P, mask)
    inputs = [fields["x"]] + [fields[k] for k in dep + helps] + [pars[k] for k in parnames] + [periodic]
    ref = numpy_nodes(model, exprs, inputs)
    assert nodes.shape == ref.shape
    for k, e in enumerate(exprs):
        assert np.array_equal(nodes[k], ref[k]), (e, np.abs(nodes[k] - ref[k]).max())


@pytest.mark.parametrize("exprs", [["U / x", "U**2 / x"], ["U / x + U**2 / x"]])
@pytest.mark.parametrize("periodic", [True, False])
def test_x_only_in_a_shared_divisor(exprs, periodic):
    """Two quotients over x: the divisor is hoisted (tf_den0 = xc) and is the only place x is read."""
    model = _model("M1_advdiff")
    N = 1003
    x = np.linspace(1.0, 3.0, N, endpoint=not periodic)
    fields = dict(x=x, U=np.cos(2 * np.pi * x) + 1.5)
    pars = dict(k=.1, c=.2)
    disc = [probes.discretise(model, e) for e in exprs]
    block, spec = codegen.lower_probes(model, disc, ["sum"] * len(exprs))
    assert spec["uses_x"] == 1 and "tf_den0 = xc;" in block
    nodes, _ = host.run(model, exprs, ["sum"] * len(exprs), x, fields, pars, periodic, 31)
    ref = numpy_nodes(model, exprs, [x, fields["U"], pars["k"], pars["c"], periodic])
    for k, e in enumerate(exprs):
        assert np.array_equal(nodes[k], ref[k]), e


def _reduce_ref(kind, f, x, dx, periodic):
    if kind == "sum":
        return math.fsum(f)
    if kind == "mean":
        return math.fsum(f) / f.size
    if kind == "integral":
        return dx * math.fsum(f) if periodic else dx * (math.fsum(f) - (f[0] + f[-1]) / 2)
    if kind in ("argmax", "argmin"):
        return x[getattr(np, kind)(f)]
    return getattr(np, kind)(f)


def _run_reductions(values, periodic, P):
    model = _model("M1_advdiff")
    N = values.size
    x = np.linspace(0.0, 3.0, N, endpoint=not periodic)
    fields = dict(x=x, U=values)
    kinds = list(probes.PROBE_REDUCTIONS)
    _, out = host.run(model, ["U"] * len(kinds), kinds, x, fields, dict(k=.1, c=.2), periodic, P)
    return dict(zip(kinds, out)), x, (x[-1] - x[0]) / (N - 1)


@pytest.mark.parametrize("N,P", [(37, 5), (1003, 31), (70001, 9000)])
@pytest.mark.parametrize("periodic", [True, False])
def test_reductions_match_numpy(N, P, periodic):
    rng = np.random.default_rng(N)
    f = rng.standard_normal(N) * np.exp(rng.uniform(-3, 3, N))
    got, x, dx = _run_reductions(f, periodic, P)
    for kind in ("max", "min", "argmax", "argmin"):
        assert got[kind] == _reduce_ref(kind, f, x, dx, periodic), kind
    for kind in ("sum", "mean", "integral"):
        ref = _reduce_ref(kind, f, x, dx, periodic)
        scale = math.fsum(np.abs(f)) * (dx if kind == "integral" else 1) / (N if kind == "mean" else 1)
        assert abs(got[kind] - ref) <= 1e-14 * scale, kind


def test_ties_follow_numpy():
    N = 1003
    f = np.zeros(N)
    f[[17, 400, 999]] = 5.0           # three maxima: the first one wins
    f[[3, 500, 1002]] = -2.0          # three minima
    got, x, _ = _run_reductions(f, False, 31)
    assert got["argmax"] == x[17] == x[np.argmax(f)]
    assert got["argmin"] == x[3] == x[np.argmin(f)]
    assert got["max"] == 5.0 and got["min"] == -2.0


def test_nan_follows_numpy():
    N = 1003
    f = np.linspace(-1, 1, N)
    f[[250, 700]] = np.nan
    got, x, _ = _run_reductions(f, True, 31)
    for kind in ("max", "min", "sum", "mean", "integral"):
        assert np.isnan(got[kind]), kind
    assert got["argmax"] == x[np.argmax(f)] == x[250]
    assert got["argmin"] == x[np.argmin(f)] == x[250]


# ---- validation --------------------------------------------------------------------------------
def _sim(name="M2_diff", N=50):
    model = _model(name)
    fields = corpus.synthetic_fields(name, N)
    return Simulation(model, fields, corpus.synthetic_pars(name, N, True), dt=1e-3,
                      time_stepping=False)


def test_unknown_reduction_is_a_value_error():
    with pytest.raises(ValueError, match="reduction"):
        _sim().add_probe("p", "U", reduce="median")


@pytest.mark.parametrize("expr", ["U *", "foo * U", "bar(U)", "dxk"])
def test_badly_formed_or_unknown_symbol(expr):
    with pytest.raises(ValueError, match="badly formated"):
        _sim().add_probe("p", expr, reduce="sum")


def test_wider_stencil_than_the_window_names_the_limit():
    with pytest.raises(UnsupportedExpression, match=r"half width 1\b"):
        _sim("M2_diff").add_probe("p", "dxxxU", reduce="max")
    with pytest.raises(UnsupportedExpression, match=r"half width 1\b"):
        _sim("M1_advdiff").add_probe("p", "dx(dxxxU)", reduce="max")


def test_model_untouched():
    model = _model("M2_diff")
    bounds, window = model._bounds, model._window_range
    footprint = {k: set(v) for k, v in model._symb_vars_with_spatial_diff_order.items()}
    src, spec = codegen.lower_model(model)
    tag = codegen.source_hash(src)
    ps = probes.ProbeSet(model)
    ps.add("a", "dxU**2 + k**3", "integral")
    ps.add("b", "U * x", "argmax")
    with pytest.raises(UnsupportedExpression):
        ps.add("c", "dxxxxU", "sum")
    assert model._bounds == bounds and model._window_range == window
    assert {k: set(v) for k, v in model._symb_vars_with_spatial_diff_order.items()} == footprint
    src2, spec2 = codegen.lower_model(model)
    assert src2 == src and codegen.source_hash(src2) == tag and spec2 == spec
    assert ps.names == ["a", "b"]


def test_probe_block_and_spec():
    model = _model("M3_film")
    disc = [probes.discretise(model, e) for e in ("h", "dxh * k**3", "x * q")]
    block, spec = codegen.lower_probes(model, disc, ["integral", "max", "argmin"])
    assert "#define TF_NPROBE 3" in block and "#define TF_PROBE_USES_X 1" in block
    assert spec["kinds"] == [2, 3, 6]
    assert "k ** 3" in spec["host_consts"]
    assert re.search(r"tf_probe_kind\[3\] = \{2, 3, 6\}", block)


def test_kernel_table_appends_the_probe_kernels():
    from triflow_amd import compilers
    with open(compilers.CSRC + "/tf_args.h") as f:
        text = f.read()
    names = re.search(r"TF_KERNEL_NAMES \{(.*?)\}", text, re.S).group(1)
    names = re.findall(r'"(tfk_\w+)"', names)
    assert names[-2:] == ["tfk_probe_partial", "tfk_probe_final"]
    assert names[27] == "tfk_poke" and names[43] == "tfk_sweep_f_stage_rhs_mon"
    assert len(names) == 46


def test_probe_that_cannot_run_is_not_kept(monkeypatch):
    """A probe set whose code object cannot be built or bound (e.g. a probe kernel that spills) is
    refused at add_probe: the probe is rolled back, the series stay readable."""
    def fail(self, solver):
        raise UnsupportedExpression("the probe kernels need more registers than a wavefront has")
    monkeypatch.setattr(probes.ProbeSet, "_bind", fail)
    import triflow_amd.simulation as simulation
    monkeypatch.setattr(simulation, "stepper_for", lambda *a, **k: _FakeStepper())
    sim = _sim()
    with pytest.raises(UnsupportedExpression):
        sim.add_probe("p", "U", reduce="max")
    assert sim.probes == {} and sim._probes.names == []


class _FakeStepper:
    class compiled:
        pars = ["k"]
    solver = None

    def bind(self, fields, pars):
        pass

    def acquire(self, fields):
        return 0


def test_probe_limit_and_empty_series():
    ps = probes.ProbeSet(_model("M2_diff"))
    for k in range(probes.MAX_PROBES):
        ps.add("p%d" % k, "U", "sum")
    with pytest.raises(ValueError, match="at most"):
        ps.add("one_more", "U", "sum")
    t, v = ps.series()["p0"]
    assert t.shape == (0,) and v.shape == (0, 1)
