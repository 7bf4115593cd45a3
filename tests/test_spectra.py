"""Device spectra on the CPU: the walk and the twiddles through the host harness (tests/spectrum_host: the
generated spectrum block and csrc/tf_spectrum.h compiled with g++) against the extended-precision referee
(tests/spectrum_cases.py), the exact identities, NaN and infinity, lowering, validation, rollback and the
host side of a set (which spectra are due, a change of solver)."""
import re

import numpy as np
import pytest

from oracle import corpus
from tests import spectrum_cases as cases
from tests.spectrum_host import build_spectrum_host as host
from tests.test_statistics import numpy_nodes
from triflow_amd import Model, _capi, codegen, compilers, probes, spectra
from triflow_amd.codegen import UnsupportedExpression
from triflow_amd.simulation import Simulation
from triflow_amd.spectra import MAX_MODES, MAX_SPECTRA

_MODELS = {}


def _model(name):
    if name not in _MODELS:
        _MODELS[name] = Model(*corpus.model_args(name), hold_compilation=True)
    return _MODELS[name]


CASES = [("M3_film", True, ["h", "We * h * dxxxh", "x"]),
         ("M1_advdiff", False, ["U", "c * dxU**2"])]
# chunks of 50 | 17 17 16 | 8 7 7 7 7 7 7 and of 53 | 18 18 17 | 9 9 9 9 9 8 nodes: one chunk, chunks of
# different lengths, lengths that are no multiple of TF_PROBE_SEG = 8, a last segment of one node (17, 9);
# 4099 (a prime) and 4100 (a multiple of four) in 5 chunks: where twiddles from a floating-point product of
# mode and node are off by more than the bound at the modes N // 4, N // 2 - 1 and N // 2
GRIDS = [(50, 1), (50, 3), (50, 7), (53, 1), (53, 3), (53, 6), (4099, 5), (4100, 5)]
WORST = dict(ratio=0.0)


def _harness(name, periodic, exprs, N, P, seed=1):
    model = _model(name)
    pars = corpus.synthetic_pars(name, N, periodic)
    fields = corpus.synthetic_fields(name, N, seed=seed, periodic=periodic)
    h = host.Harness(model, exprs, fields["x"], pars, periodic, P)
    return h, fields, numpy_nodes(model, exprs, fields, pars)


@pytest.mark.parametrize("name,periodic,exprs", CASES, ids=[c[0] for c in CASES])
@pytest.mark.parametrize("N,P", GRIDS)
def test_walk_and_twiddles_against_the_referee(name, periodic, exprs, N, P):
    h, fields, nodes = _harness(name, periodic, exprs, N, P)
    modes = cases.mode_set(N)
    assert {N // 4, N // 2 - 1, N // 2} <= set(modes)
    for which, e in enumerate(exprs):
        got = h.run(which, modes, fields)
        r = cases.ratios(got, nodes[which], modes)
        WORST["ratio"] = max(WORST["ratio"], float(r.max()))
        print("%s N=%d P=%d %s: worst |c - c_ref| / (2**-53 sum|v|) = %.3f (so far %.3f)"
              % (name, N, P, e, r.max(), WORST["ratio"]))
        assert (r <= cases.BOUND_ULPS).all(), (e, modes, r)


def test_the_issue_signal_and_what_the_bound_is_for():
    """The signal the bound was calibrated on, through the harness as the state of the advection model;
    and the error the bound exists to catch: twiddles from m * g / N formed in floating point."""
    for N in (4099, 4100):
        v = cases.signal(N)
        model = _model("M1_advdiff")
        pars = corpus.synthetic_pars("M1_advdiff", N, False)
        x = corpus.synthetic_fields("M1_advdiff", N, periodic=False)["x"]
        h = host.Harness(model, ["U"], x, pars, False, 5)
        modes = cases.mode_set(N)
        r = cases.ratios(h.run(0, modes, dict(x=x, U=v)), v, modes)
        print("signal N=%d: worst ratio %.3f" % (N, r.max()))
        assert (r <= cases.BOUND_ULPS).all(), r
        g = np.arange(N)
        naive = np.array([np.sum(v * np.exp(-2j * np.pi * m * g / N)) for m in modes])
        assert cases.ratios(naive, v, modes).max() > cases.BOUND_ULPS      # (such a build fails the test above)


@pytest.mark.parametrize("N,P", [(50, 3), (53, 6), (4100, 5)])
def test_exact_identities(N, P):
    name, periodic, exprs = CASES[0]
    h, fields, _ = _harness(name, periodic, exprs, N, P)
    modes = [0, 1, N // 4, N // 2]
    for which in range(len(exprs)):
        got = h.run(which, modes, fields)
        assert got[0].imag == 0 and np.float64(got[0].imag).tobytes() == np.float64(0.0).tobytes()     # mode 0
        assert got[1].imag != 0
        if N % 2 == 0:
            assert got[3].imag == 0                                          # mode N / 2 of an even N
    one = np.array([1.0, 0.0]).tobytes()
    assert np.array(host.twiddle(h.lib, 0, N)).tobytes() == one
    if N % 2 == 0:
        assert np.array(host.twiddle(h.lib, N // 2, N)).tobytes() == np.array([-1.0, 0.0]).tobytes()
    if N % 4 == 0:
        assert np.array(host.twiddle(h.lib, N // 4, N)).tobytes() == np.array([0.0, -1.0]).tobytes()
        assert np.array(host.twiddle(h.lib, 3 * N // 4, N)).tobytes() == np.array([0.0, 1.0]).tobytes()


def test_twiddle_function_alone():
    """At most 2 * 2**-53 in each part: the rounding of the argument plus one libm call."""
    lib = _harness(*CASES[1], 50, 1)[0].lib
    worst = 0.0
    for N in (53, 4100):
        c, s = cases.twiddle_table(N)
        got = np.array([host.twiddle(lib, r, N) for r in range(N)])
        err = max(np.abs(got[:, 0].astype(np.longdouble) - c).max(), np.abs(got[:, 1].astype(np.longdouble) - s).max())
        worst = max(worst, float(err / cases.UNIT))
    N = 2 ** 31 - 1
    for r in np.random.RandomState(7).randint(0, N, 1000):
        a, b = host.twiddle(lib, r, N)
        c, s = cases.twiddle_exact(r, N)
        worst = max(worst, float(max(abs(np.longdouble(a) - c), abs(np.longdouble(b) - s)) / cases.UNIT))
    print("twiddle function: worst error %.3f * 2**-53" % worst)
    assert worst <= 2.0


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_nan_and_infinity_reach_every_mode(bad):
    """One node that is not finite makes every mode of the row NaN in both parts.  (np.fft.fft is less
    uniform: at these sizes an infinity leaves infinities of either sign, NaNs and, at mode 0, a zero
    imaginary part, depending on the factorisation of N.)"""
    name, periodic, exprs = CASES[1]
    N, P = 53, 6
    h, fields, _ = _harness(name, periodic, exprs, N, P)
    modes = cases.mode_set(N)
    fields = dict(fields, U=np.array(fields["U"]))
    fields["U"][20] = bad
    got = h.run(0, modes, fields)
    assert np.isnan(got.real).all() and np.isnan(got.imag).all(), got


# ---- lowering ----------------------------------------------------------------------------------
def test_spectrum_block_and_spec():
    model = _model("M3_film")
    disc = [probes.discretise(model, e) for e in ("h", "dxh * k**3", "x * q")]
    block, spec = codegen.lower_spectra(model, disc)
    assert "#define TF_NSPEC 3" in block and "#define TF_SPEC_USES_X 1" in block and "#define TF_NSPEC_HC 1" in block
    assert "tf_eval_spectrum(int k," in block and spec["nspec"] == 3
    rblock, rspec = codegen.lower_records(model, disc)
    assert rspec["host_consts"] == spec["host_consts"] and rspec["uses_x"] == spec["uses_x"]
    lines = [ln for ln in rblock.splitlines() if ln.startswith("    case ")]
    assert len(lines) == 3 and lines == [ln for ln in block.splitlines() if ln.startswith("    case ")]
    with pytest.raises(UnsupportedExpression, match="Heaviside"):
        codegen.lower_spectra(model, [probes.discretise(model, "Heaviside(h - 1)")])


def test_the_spectrum_kernels_follow_the_table():
    with open(compilers.CSRC + "/tf_args.h") as f:
        text = f.read()
    # what the tests of the other observers pin stays as it was
    assert 'TF_KERNEL_NAMES_STAT { "tfk_stat" }' in text and "TFK_STAT = TFK_COUNT" in text
    assert re.search(r"TFK_PROBE_FINAL,\s*TFK_RECORD, TFK_COUNT", text)
    assert 'TF_KERNEL_NAMES_SPECTRUM { "tfk_spectrum_partial", "tfk_spectrum_final" }' in text
    assert int(re.search(r"#define TF_SPEC_MAX_MODES (\d+)", text).group(1)) == MAX_MODES >= 64
    assert "tf_rt_spectrum.cpp" in compilers.RUNTIME_SOURCES    # (the code objects: tests/test_observer_objects.py)
    assert spectra.SpectrumSet.kind == "spectrum"
    with pytest.raises(ValueError, match="kind of observer"):
        compilers.build_observer_code_object(_model("M2_diff"), "", "statistic")
    names = _capi.Library(compilers.build_runtime_library()).kernel_names()
    at = names.index("tfk_stat")
    assert names[at + 1:at + 3] == ["tfk_spectrum_partial", "tfk_spectrum_final"] and len(names) <= 64


def test_spectrum_is_a_kind_of_observer_code_object_and_does_not_spill():
    model = _model("M2_diff")
    block, _ = codegen.lower_spectra(model, [probes.discretise(model, "U"), probes.discretise(model, "k * dxxU")])
    hsaco = compilers.build_observer_code_object(model, block, "spectrum")
    usage = compilers.resource_usage(hsaco)
    for kernel in ("tfk_spectrum_partial", "tfk_spectrum_final"):
        assert usage[kernel]["ScratchSize"] == 0 and usage[kernel]["VGPRs"] > 0, (kernel, usage[kernel])


# ---- validation --------------------------------------------------------------------------------
def _sim(name="M2_diff", N=50):
    model = _model(name)
    fields = corpus.synthetic_fields(name, N)
    return Simulation(model, fields, corpus.synthetic_pars(name, N, True), dt=1e-3, time_stepping=False)


@pytest.mark.parametrize("kwargs,match", [
    (dict(modes=[]), "empty"),
    (dict(modes=range(0)), "empty"),
    (dict(modes=5), "sequence"),
    (dict(modes=[1, 2.0]), "not an integer"),
    (dict(modes=[1.5]), "not an integer"),
    (dict(modes=[0, True]), "not an integer"),
    (dict(modes=["1"]), "not an integer"),
    (dict(modes=[-1]), "outside"),
    (dict(modes=[0, 26]), "outside"),
    (dict(modes=[3, 4, 3]), "twice"),
    (dict(modes=[1], every=0), "every"),
    (dict(modes=[1], every=1.5), "every"),
    (dict(modes=[1], every=True), "every"),
    (dict(modes=[1], capacity=0), "capacity"),
])
def test_validation_errors(kwargs, match):
    with pytest.raises(ValueError, match=match) as err:
        _sim().add_spectrum("s", "U", **kwargs)
    assert "spectrum" in str(err.value)


def test_more_modes_than_the_tables_hold():
    ss = spectra.SpectrumSet(_model("M2_diff"), 4100)
    with pytest.raises(ValueError, match="at most %d" % MAX_MODES) as err:
        ss.add("s", "U", modes=range(MAX_MODES + 1))
    assert "spectrum" in str(err.value)
    ss.add("s", "U", modes=range(MAX_MODES))
    ss.add("np", "U", modes=np.arange(3, dtype=np.int32))
    assert ss._items[1].modes == [0, 1, 2]


@pytest.mark.parametrize("expr", ["U *", "foo * U", "bar(U)", "dxk", 3])
def test_badly_formed_or_unknown_symbol(expr):
    with pytest.raises(ValueError, match="badly formated"):
        _sim().add_spectrum("s", expr, modes=[1])


def test_heaviside_is_refused():
    with pytest.raises(UnsupportedExpression, match="Heaviside"):
        _sim().add_spectrum("s", "Heaviside(U - 1) * U", modes=[1])


def test_duplicate_names_removal_and_the_limit():
    ss = spectra.SpectrumSet(_model("M2_diff"), 50)
    ss.add("a", "U", modes=range(5), every=3)
    with pytest.raises(ValueError, match="spectrum named 'a' exists already"):
        ss.add("a", "dxU", modes=[1])
    ss.add("b", "dxU", modes=[25])
    ss.add("c", "U", modes=[7, 3])                         # same expression, other modes: the same case
    assert ss.names == ["a", "b", "c"] and len(ss.expressions()) == 2
    assert ss._lower(0)[0] == spectra.SpectrumSet._lower(_two_expression_set(), 0)[0]
    ss.remove("a")
    assert ss.names == ["b", "c"]
    with pytest.raises(KeyError):
        ss.remove("a")
    with pytest.raises(KeyError):
        _sim().remove_spectrum("nope")
    t, k, c = ss.series(per_system=False)["b"]
    assert t.shape == (0,) and k.shape == (1,) and c.shape == (0, 1) and c.dtype == np.complex128
    assert _sim().spectra == {}
    for i in range(MAX_SPECTRA - 2):
        ss.add("s%d" % i, "U", modes=[i % 20])
    assert len(ss.names) == MAX_SPECTRA == 64
    with pytest.raises(ValueError, match="at most 64 spectra") as err:
        ss.add("one more", "U", modes=[1])
    assert "spectrum" in str(err.value)


def _two_expression_set():
    """The same two expressions with other modes: the block (and so the code object) is the same."""
    ss = spectra.SpectrumSet(_model("M2_diff"), 50)
    ss.add("p", "U", modes=[11])
    ss.add("q", "dxU", modes=[0, 1, 2])
    return ss


# ---- the host side of a set ----------------------------------------------------------------------
class _FakeStepper:
    class compiled:
        pars = ["k"]
    solver = None

    def bind(self, fields, pars):
        pass

    def acquire(self, fields):
        return 0


def test_spectrum_that_cannot_run_is_not_kept(monkeypatch):
    def fail(self, solver):
        raise UnsupportedExpression("the spectrum kernels need more registers than a wavefront has")
    import triflow_amd.simulation as simulation
    monkeypatch.setattr(simulation, "stepper_for", lambda *a, **k: _FakeStepper())
    sim = _sim()
    ss = sim._spectra = spectra.SpectrumSet(sim.model, 50)
    ss.add("kept", "U", modes=[0, 1])
    kept = ss._items[0]
    kept.last = kept.origin = sim.i
    kept.t, kept.blocks, kept.k = [0.0], [np.arange(2.0).reshape(1, 1, 2).astype(np.complex128)], np.array([0.0, 1.0])
    monkeypatch.setattr(spectra.SpectrumSet, "_bind", fail)
    with pytest.raises(UnsupportedExpression):
        sim.add_spectrum("s", "U", modes=[3])
    assert list(sim.spectra) == ["kept"] and sim._spectra.names == ["kept"]
    t, k, c = sim.spectra["kept"]
    assert np.array_equal(t, [0.0]) and np.array_equal(c, np.arange(2.0).reshape(1, 2))
    assert sim.probes == {} and sim.recorders == {} and sim.statistics == {}
    sim.remove_spectrum("kept")
    with pytest.raises(UnsupportedExpression):
        sim.add_spectrum("s", "U", modes=[3])
    assert sim.spectra == {} and sim._spectra.names == []


class _Handle:
    """Stands in for _capi.DeviceSpectrum: a row holds the number of the record, the calls are kept."""

    def __init__(self, solver, nmodes):
        self.solver, self.calls, self.rows, self.nmodes = solver, [], {}, nmodes

    def set_x(self, x):
        pass

    def record(self, k, slot):
        self.calls.append(("record", k))
        self.rows.setdefault(k, []).append(float(len(self.calls)))

    def fetch(self, k):
        self.calls.append(("fetch", k))
        rows = self.rows.pop(k, [])
        return np.array(rows, dtype=np.complex128).reshape(-1, 1, 1) * np.ones((1, 1, self.nmodes[k]))

    def close(self):
        pass


class _Solver:
    nsys, N = 1, 50

    class model:
        spec = dict(uses_x=0)


def _fake_set():
    ss = spectra.SpectrumSet(_model("M2_diff"), 50)
    bounds = {}

    def bind(solver):
        if solver.N != ss.N:
            return spectra.SpectrumSet._bind(ss, solver)
        if id(solver) not in bounds:
            bounds[id(solver)] = spectra._Bound(_Handle(solver, [len(r.modes) for r in ss._items]), dict(host_consts=[]))
        return bounds[id(solver)]
    ss._bind = bind
    return ss, bounds


def test_only_spectra_that_are_due_are_launched():
    ss, bounds = _fake_set()
    x = np.linspace(0, 2, 50)
    solver = _Solver()
    ss.add("every1", "U", modes=[0, 1, 2])
    assert ss.due(4) == [0]
    ss.record(solver, 0, 0.4, 4, x, [[1.0]])
    assert ss.due(4) == [] and ss.due(5) == [0]
    ss.add("every3", "U", modes=[5], every=3)
    bounds.clear()                                         # (add closed the handles: a new one is bound)
    assert ss.due(4) == [1]
    ss.record(solver, 0, 0.4, 4, x, [[1.0]])               # (the first row of the new one only)
    handle = bounds[id(solver)].handle
    assert handle.calls == [("record", 1)]
    dues = []
    for key in range(5, 12):
        dues.append(ss.due(key))
        ss.record(solver, 0, 0.1 * key, key, x, [[1.0]])
        ss.record(solver, 0, 0.1 * key, key, x, [[1.0]])   # (the same state again: no second row)
    assert dues == [[0], [0], [0, 1], [0], [0], [0, 1], [0]]
    assert [c[1] for c in handle.calls if c[0] == "record"] == [1, 0, 0, 0, 1, 0, 0, 0, 1, 0]
    s = ss.series(per_system=False)
    t1, k1, c1 = s["every1"]
    t3, k3, c3 = s["every3"]
    assert c1.shape == (8, 3) and c3.shape == (3, 1)
    assert np.allclose(t1, [0.4] + [0.1 * k for k in range(5, 12)]) and np.allclose(t3, [0.4, 0.7, 1.0])
    dx = 2.0 / 49
    assert np.array_equal(k1, 2.0 * np.pi * np.array([0.0, 1.0, 2.0]) / (50 * ((x[-1] - x[0]) / 49)))
    assert np.allclose(k3, 2 * np.pi * 5 / (50 * dx))
    assert np.array_equal(c3[:, 0].real, [1.0, 5.0, 9.0])  # in record order


def test_a_change_of_solver_loses_no_row_and_another_grid_is_refused():
    ss, bounds = _fake_set()
    x = np.linspace(0, 1, 50)
    first, second = _Solver(), _Solver()
    ss.add("m", "U", modes=[1, 2])
    for key in range(4):
        ss.record(first, 0, 0.1 * key, key, x, [[1.0]])
    for key in range(4, 7):
        ss.record(second, 0, 0.1 * key, key, x, [[1.0]])
    t, k, c = ss.series(per_system=False)["m"]
    assert c.shape == (7, 2) and np.array_equal(c[:, 0].real, [1, 2, 3, 4, 1, 2, 3])
    assert np.allclose(t, 0.1 * np.arange(7))

    class Other(_Solver):
        N = 60
    with pytest.raises(ValueError, match="laid out for 50 nodes") as err:
        ss.record(Other(), 0, 0.7, 7, np.linspace(0, 1, 60), [[1.0]])
    assert "spectrum" in str(err.value)
    assert ss.series(per_system=False)["m"][2].shape == (7, 2)


def test_ensemble_wavenumbers_follow_the_recorders_rule_for_x():
    ss, bounds = _fake_set()

    class Eight(_Solver):
        nsys = 8
    ss.add("m", "U", modes=[0, 3])
    x = np.linspace(0, 1, 50)
    ss.record(Eight(), 0, 0.0, 0, np.tile(x, (8, 1)), [[1.0]] * 8)
    ss._items[0].pending.clear()
    assert ss.series()["m"][1].shape == (2,)
    ss2, _ = _fake_set()
    ss2.add("m", "U", modes=[0, 3])
    xs = np.array([x * (1 + e) for e in range(8)])
    ss2.record(Eight(), 0, 0.0, 0, xs, [[1.0]] * 8)
    ss2._items[0].pending.clear()
    k = ss2.series()["m"][1]
    assert k.shape == (8, 2) and np.allclose(k[:, 1] * (1 + np.arange(8)), k[0, 1])
    assert ss2.series(per_system=False)["m"][1].shape == (2,)
