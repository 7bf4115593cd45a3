"""The function vocabulary of the generated code on the MI355X: the table of tests/vocab_cases.py through
the HIP path (``Model``, the recorders and probes of a ``Simulation``, the F / J kernels) against mpmath,
and the bytes of every exact-class expression against the host build of the same generated code.

The recorder is the instrument of the function cases: ``pool="sample"`` over every node returns the raw
per-node value of the expression; the t0 row is written when the set first records, no step is taken."""
import math

import numpy as np
import pytest

from tests import vocab_cases as vc
from triflow_amd import Model, Simulation, compilers, probes, recorders
from triflow_amd.codegen import UnsupportedExpression
from triflow_amd.ensemble import Ensemble

pytestmark = pytest.mark.gpu

_CARRIER = []
_ROWS = {}


def carrier():
    if not _CARRIER:
        _CARRIER.append(Model(*vc.CARRIER))
    return _CARRIER[0]


@pytest.fixture(autouse=True)
def sympy_objects_pass(monkeypatch):
    """log2, log10, log1p, expm1 have no spelling in the string language: the cases hand the recorders the
    SymPy objects (tests/vocab_cases.py::discretise)."""
    monkeypatch.setattr(recorders, "discretise", vc.discretise)


def simulation_of(case, periodic=True):
    st = case.state()
    fields = dict(x=vc.carrier_x(periodic), U=st["U"], V=st["V"], W=st["W"])
    return Simulation(carrier(), fields, dict(k=st["k"], c=st["c"], periodic=periodic), dt=1e-3, time_stepping=False)


def record_group(sim, gname):
    """The recorders of a whole group on ``sim``'s state: the t0 rows, name -> [NARG].  (The set is built
    first and attached: ``add_recorder`` one by one would compile the growing set once per recorder.)"""
    rs = recorders.RecorderSet(sim.model, vc.NARG)
    for c in vc.FUNCTION_GROUPS[gname][0]:
        rs.add(c.name, c.expr)
    sim._recorders = rs
    sim._record_on(rs)
    return {name: values[0] for name, (t, x, values) in sim.recorders.items()}


def device_row(gname, case):
    """The row of ``case`` on its own argument set, recorded once per session.  (Every case has a state of
    its own, so the group's set records once per case; only the case's row is kept, the simulation and
    its device rings are released.)"""
    key = (gname, case.name)
    if key not in _ROWS:
        sim = simulation_of(case)
        _ROWS[key] = np.array(record_group(sim, gname)[case.name])
        sim._recorders.close()
    return _ROWS[key]


def _cases(*kinds):
    return [pytest.param(g, c, id="%s-%s" % (g, c.name)) for g, (cases, _) in vc.FUNCTION_GROUPS.items()
            for c in cases if c.kind in kinds]


# ---- exact class -------------------------------------------------------------------------------
@pytest.mark.parametrize("gname,case", _cases("op", "exact", "divu", "powi", "npowi", "hostc"))
def test_exact_class_has_the_bytes_of_the_host_build(gname, case):
    """IEEE operations and FMAs only: a difference is a contraction or a miscompile."""
    got, host = device_row(gname, case), vc.host_row(gname, case)
    assert got.tobytes() == host.tobytes(), (case, np.flatnonzero(got != host)[:5])


@pytest.mark.parametrize("gname,case", _cases("op", "exact", "divu", "hostc"))
def test_exact_class_has_the_bytes_of_numpy(gname, case):
    got = device_row(gname, case)
    exact, ref = vc.case_references(gname, case)
    if case.kind == "divu":
        # csrc/tf_math.h (tf_div_u): IEEE division but for a divisor whose significand is all ones, where
        # the header promises a result within one ulp
        ones = vc.is_all_ones(case.state()["V"])
        assert ones.sum() >= 200
        assert got[~ones].tobytes() == ref[~ones].tobytes(), case
        err = vc.ulp_errors(got[ones], [e for e, o in zip(exact, ones) if o])
        print(case, "all-ones divisors: worst %.3f ulp, %d of %d differ from IEEE division"
              % (err.max(), (got[ones] != ref[ones]).sum(), ones.sum()))
        assert err.max() <= 1.0, case
        return
    assert got.tobytes() == ref.tobytes(), (case, np.flatnonzero(got != ref)[:5])
    if case.kind == "op":
        err = vc.ulp_errors(got, exact)
        assert err.max() <= 0.5, (case, err.max())


def test_sign_of_negative_zero_is_numpys():
    case = [c for c in vc.EXACT_GROUP if c.name == "sign"][0]
    u, got = case.state()["U"], device_row("exact", case)
    zeros = (u == 0) & np.signbit(u)
    assert zeros.sum() >= 40 and not np.signbit(got[zeros]).any()
    assert got.tobytes() == np.sign(u).tobytes()


@pytest.mark.parametrize("gname,case", _cases("powi"))
def test_integer_powers_are_correctly_rounded(gname, case):
    got = device_row(gname, case)
    exact, _ = vc.case_references(gname, case)
    assert vc.not_nearest(got, exact) == [], case


@pytest.mark.parametrize("gname,case", _cases("npowi"))
def test_reciprocal_powers(gname, case):
    got, host = device_row(gname, case), vc.host_row(gname, case)
    exact, _ = vc.case_references(gname, case)
    err = vc.ulp_errors(got, exact)
    share, host_share = len(vc.not_nearest(got, exact)) / got.size, len(vc.not_nearest(host, exact)) / got.size
    print(case, "worst %.3f ulp, not correctly rounded: device %.4f host %.4f" % (err.max(), share, host_share))
    assert err.max() <= 1.0, case
    assert share <= host_share, case


# ---- libm class --------------------------------------------------------------------------------
@pytest.mark.parametrize("gname,case", _cases("libm"))
def test_libm_class_within_the_measured_bound(gname, case):
    got = device_row(gname, case)
    exact, ref = vc.case_references(gname, case)
    err = vc.ulp_errors(got, exact)
    worst = int(err.argmax())
    print("%-20s device %.3f ulp at u = %r   NumPy %.3f ulp" % (case.name, err.max(), case.state()["U"][worst],
                                                               vc.ulp_errors(ref, exact).max()))
    assert err.max() <= vc.libm_bound(case.fn, device=True), (case, err.max())


# ---- the public entry points ---------------------------------------------------------------------
def test_function_cases_through_add_recorder():
    """``Simulation.add_recorder`` itself (the tests above attach a whole set at once): a libm case and
    an exact case, one code object each, against the rows of the attached set."""
    for gname, name, expr in (("libm", "sin", "sin(U)"), ("exact", "sign", "sign(U)")):
        case = [c for c in vc.FUNCTION_GROUPS[gname][0] if c.name == name][0]
        sim = simulation_of(case)
        sim.add_recorder("r", expr)
        t, x, values = sim.recorders["r"]
        assert values.shape == (1, vc.NARG) and np.array_equal(x, vc.carrier_x())
        assert values[0].tobytes() == device_row(gname, case).tobytes(), name
        exact, _ = vc.case_references(gname, case)
        assert vc.ulp_errors(values[0], exact).max() <= (vc.libm_bound("sin", True) if name == "sin" else 0.0)
        sim.remove_recorder("r")


def test_total_variation_through_add_probe():
    N, periodic = 20011, False
    x, U = vc.probe_state(N, periodic)
    sim = Simulation(carrier(), dict(x=x, U=U, V=U + 1, W=U + 2), dict(k=0.75, c=1.25, periodic=periodic), dt=1e-3,
                     time_stepping=False)
    sim.add_probe("tv", "Abs(dxU)", reduce="sum")
    oracle = vc.carrier_model()
    exact = vc.exact_nodes(oracle, [vc.discretise(oracle, "Abs(dxU)")], [x, U, U + 1, U + 2, 0.75, 1.25, periodic])[0]
    f = np.array([float(v) for v in exact])
    t, values = sim.probes["tv"]
    assert values.shape == (1,) and abs(values[0] - math.fsum(f)) <= 1e-14 * math.fsum(np.abs(f))


# ---- host constants ----------------------------------------------------------------------------
def test_host_constants_are_numpys_values():
    k = vc.HOSTC_GROUP[0].state()["k"]
    want = dict(zip(("exp(k)", "log(k+2)", "k**3"), (np.exp(np.float64(k)), np.log(np.float64(k) + 2), np.float64(k) ** 3)))
    for case in vc.HOSTC_GROUP[:3]:
        got = device_row("hostc", case)
        assert got.tobytes() == np.full(vc.NARG, want[case.name]).tobytes(), case


def test_every_ensemble_member_gets_its_own_constants():
    model, nsys = carrier(), 5
    st = vc.HOSTC_GROUP[0].state()
    ks = np.array([0.8125, -0.3, 1.7, 2.0 ** -20, 3.25])
    fdict = {v: np.tile(st[v], (nsys, 1)) for v in "UVW"}
    ens = Ensemble(model, vc.carrier_x(), fdict, dict(k=ks, c=1.25), periodic=True, scheme="ROS2")
    rs = recorders.RecorderSet(model, vc.NARG)           # (the set of the "hostc" group: one code object)
    for c in vc.HOSTC_GROUP:
        rs.add(c.name, c.expr)
    ens._recorders = rs
    ens._record_on(rs)
    got = ens.recorders
    ens.close()
    oracle = vc.carrier_model()
    disc = [vc.discretise(oracle, c.expr) for c in vc.HOSTC_GROUP]
    for e, k in enumerate(ks):
        for name, want in (("exp(k)", np.exp(k)), ("log(k+2)", np.log(k + 2)), ("k**3", k ** 3)):
            row = got[name][2][0, e]
            assert row.tobytes() == np.full(row.size, want).tobytes(), (name, e)
        ref = vc.numpy_nodes(oracle, disc, vc.carrier_inputs(dict(st, k=k, c=1.25)))
        for c, r in zip(vc.HOSTC_GROUP, ref):
            assert got[c.name][2][0, e].tobytes() == r.tobytes(), (c, e)


# ---- probes ------------------------------------------------------------------------------------
@pytest.mark.parametrize("periodic", [True, False])
def test_probes_of_the_helpers(periodic):
    N = 20011
    x, U = vc.probe_state(N, periodic)
    model = carrier()
    sim = Simulation(model, dict(x=x, U=U, V=U + 1, W=U + 2), dict(k=0.75, c=1.25, periodic=periodic), dt=1e-3,
                     time_stepping=False)
    ps = probes.ProbeSet(model)                          # (built first and attached, as record_group does)
    for n, (expr, kind) in enumerate(vc.PROBE_CASES):
        ps.add("p%d" % n, expr, kind)
    sim._probes = ps
    sim._record_on(ps)
    got = sim.probes
    oracle = vc.carrier_model()
    disc = [vc.discretise(oracle, e) for e, _ in vc.PROBE_CASES]
    exact = vc.exact_nodes(oracle, disc, [x, U, U + 1, U + 2, 0.75, 1.25, periodic])
    dx = (x[-1] - x[0]) / (N - 1)
    for n, (expr, kind) in enumerate(vc.PROBE_CASES):
        f = np.array([float(v) for v in exact[n]])
        g, ref = got["p%d" % n][1][0], vc.reduce_exact(kind, f, x, dx, periodic)
        print(expr, kind, g, ref)
        if kind in ("sum", "mean", "integral"):
            assert abs(g - ref) <= 1e-14 * vc.reduce_scale(kind, f, dx), (expr, kind, g, ref)
        else:
            assert g == ref, (expr, kind, g, ref)


# ---- models ------------------------------------------------------------------------------------
@pytest.mark.parametrize("per_node", [False, True], ids=["scalar", "per-node"])
@pytest.mark.parametrize("periodic", [True, False], ids=["periodic", "clamped"])
@pytest.mark.parametrize("name", sorted(vc.MODEL_CASES))
def test_model_cases(name, periodic, per_node):
    vc.check_model_case(name, None, periodic, per_node)


# ---- refusals ----------------------------------------------------------------------------------
@pytest.mark.parametrize("expr,match", vc.REFUSED)
def test_refused_observers_leave_the_simulation_usable(expr, match):
    x, U = vc.probe_state(vc.NARG, True)
    sim = Simulation(carrier(), dict(x=x, U=U, V=U + 1, W=U + 2), dict(k=1e-3, c=1.25, periodic=True), dt=1e-3,
                     time_stepping=False)
    builds = compilers.BUILD_COUNT
    with pytest.raises(UnsupportedExpression, match=match):
        sim.add_recorder("r", expr)
    with pytest.raises(UnsupportedExpression, match=match):
        sim.add_probe("p", expr, reduce="max")
    assert compilers.BUILD_COUNT == builds and sim.recorders == {} and sim.probes == {}
    sim.add_recorder("u", "U", nodes=slice(None, None, 100))
    next(sim)
    t, x, values = sim.recorders["u"]
    assert values.shape == (2, math.ceil(vc.NARG / 100)) and np.isfinite(values).all()
