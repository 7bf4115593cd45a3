"""The function vocabulary of the generated code on the CPU: the table of tests/vocab_cases.py through the
host builds of the same generated code (models: tests/emu; recorders and probes: tests/record_host,
tests/probe_host) against mpmath.  glibc does the libm calls here, so this tier tests the *lowering*: the
operation tree, the hoisting of divisors, the host constants, the plumbing of per-node parameters and
of ``x``.  tests/test_gpu_vocabulary.py runs the same table through the HIP path."""
import os

import numpy as np
import pytest

from tests import vocab_cases as vc
from tests.emu import build_emu
from tests.probe_host import build_probe_host as phost
from triflow_amd import Model, codegen, compilers, recorders
from triflow_amd.codegen import UnsupportedExpression
from triflow_amd.simulation import Simulation


@pytest.fixture(scope="module")
def backend():
    # -O0: half the compile time of a library that is built once per case, and the same IEEE arithmetic
    # (no contraction, no fast-math at either level)
    return build_emu.EmuBackend(opt="-O0")


_ROWS = {}


def rows(gname, case):
    """(host build's values, exact values, NumPy's values) of a function case, computed once."""
    key = (gname, case.name)
    if key not in _ROWS:
        _ROWS[key] = (vc.host_row(gname, case), *vc.case_references(gname, case))
    return _ROWS[key]


def _cases(*kinds):
    return [pytest.param(g, c, id="%s-%s" % (g, c.name)) for g, (cases, _) in vc.FUNCTION_GROUPS.items()
            for c in cases if c.kind in kinds]


# ---- the lowering the cases are there for -------------------------------------------------------
def test_the_groups_lower_to_the_forms_they_name():
    def line(gname, case):
        block = vc.host_group(gname)[2]
        k = vc.FUNCTION_GROUPS[gname][0].index(case)
        return [ln for ln in block.splitlines() if ln.startswith("    case %d: return" % k)][0]
    by = {c.name: (g, c) for g, (cases, _) in vc.FUNCTION_GROUPS.items() for c in cases}
    for name, token in (("u**0.5", "sqrt(v_U)"), ("u**-1", "(1.0 / v_U)"), ("u**2", "tf_sq(v_U)"), ("u**7", "tf_powi(v_U, 7)"),
                        ("u**-16", "tf_powi(v_U, -16)"), ("u**1.5", "pow(v_U, 0x1.8"), ("2**u", "pow(2.0, v_U)"),
                        ("u**u", "pow(v_U, v_U)"), ("u**k", "pow(v_U, v_k)"), ("sign", "tf_sign(v_U)"),
                        ("max3", "tf_max(tf_max("), ("u/k", "tf_div_u(v_U, tf_den"), ("u/x", "(v_U / xc)"),
                        ("u/v", "tf_div_u(v_U, tf_den"), ("w/v", "tf_div_u(v_W, tf_den"), ("exp(k)", "tf_hc[0]"),
                        ("exp(k) per node", "exp(v_k)"), ("k**3 per node", "tf_powi(v_k, 3)"), ("log2", "log2(v_U)"),
                        ("expm1", "expm1(v_U)"), ("ceil", "ceil(v_U)")):
        assert token in line(*by[name]), (name, line(*by[name]))
    assert line(*by["shared"]).count("tf_div_u(") == 2 and "(v_U / (tf_sq(v_U) + 1.0))" in line(*by["shared"])
    assert vc.host_group("hostc")[1]["host_consts"] == ["exp(k)", "log(k + 2)", "k ** 3", "c ** 3"]
    assert "#define TF_REC_USES_X 1" in vc.host_group("exact")[2]         # (x only in "u/x")


# ---- exact class -------------------------------------------------------------------------------
@pytest.mark.parametrize("gname,case", _cases("op", "exact", "divu", "hostc"))
def test_exact_class_has_the_bytes_of_numpy(gname, case):
    got, exact, ref = rows(gname, case)
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
        assert vc.ulp_errors(got, exact).max() <= 0.5, case


def test_sign_of_negative_zero_is_numpys():
    case = [c for c in vc.EXACT_GROUP if c.name == "sign"][0]
    u, got = case.state()["U"], rows("exact", case)[0]
    zeros = (u == 0) & np.signbit(u)
    assert zeros.sum() >= 40 and not np.signbit(got[zeros]).any()
    assert got.tobytes() == np.sign(u).tobytes()


def test_max_min_of_signed_zeros_are_numpys():
    for name, fn in (("max2", np.maximum), ("min2", np.minimum)):
        case = [c for c in vc.EXACT_GROUP if c.name == name][0]
        st, got = case.state(), rows("exact", case)[0]
        assert list(np.signbit(st["U"][:2])) == [False, True] and list(np.signbit(st["V"][:2])) == [True, False]
        assert (st["U"][:16] == 0).all() and (st["V"][:16] == 0).all()
        # the second operand comes back (SymPy prints Max(U, V) in this order)
        assert got[:16].tobytes() == fn(st["U"], st["V"])[:16].tobytes() == st["V"][:16].tobytes()


@pytest.mark.parametrize("gname,case", _cases("powi"))
def test_integer_powers_are_correctly_rounded(gname, case):
    got, exact, _ = rows(gname, case)
    assert vc.not_nearest(got, exact) == [], case


@pytest.mark.parametrize("gname,case", _cases("npowi"))
def test_reciprocal_powers_within_one_ulp(gname, case):
    got, exact, _ = rows(gname, case)
    assert vc.ulp_errors(got, exact).max() <= 1.0, case


# ---- libm class --------------------------------------------------------------------------------
@pytest.mark.parametrize("gname,case", _cases("libm"))
def test_libm_class_within_the_measured_bound(gname, case):
    got, exact, _ = rows(gname, case)
    err = vc.ulp_errors(got, exact)
    print("%-20s host build %.3f ulp at u = %r" % (case.name, err.max(), case.state()["U"][int(err.argmax())]))
    assert err.max() <= vc.libm_bound(case.fn, device=False), (case, err.max())


@pytest.mark.parametrize("gname,case", _cases("op", "divu", "powi", "npowi", "libm"))
def test_numpy_stays_within_two_ulp_on_the_argument_sets(gname, case):
    """The argument sets do not break the yardstick the model cases lean on."""
    _, exact, ref = rows(gname, case)
    assert vc.ulp_errors(ref, exact).max() <= 2.0, case


def test_every_bound_follows_the_rule():
    for fn, (dev, host) in vc.MEASURED_ULP.items():
        assert dev <= 3 and host <= 3, fn                   # (above 3 ulp: a finding)
        assert vc.libm_bound(fn, True) <= vc.LIBM_CAP and vc.libm_bound(fn, False) <= vc.LIBM_CAP
    used = {c.fn for cases, _ in vc.FUNCTION_GROUPS.values() for c in cases if c.kind == "libm"}
    assert used == set(vc.MEASURED_ULP)


# ---- host constants ----------------------------------------------------------------------------
def test_host_constants_are_numpys_values():
    k = np.float64(vc.HOSTC_GROUP[0].state()["k"])
    want = {"exp(k)": np.exp(k), "log(k+2)": np.log(k + 2), "k**3": k ** 3}
    for case in vc.HOSTC_GROUP[:3]:
        assert rows("hostc", case)[0].tobytes() == np.full(vc.NARG, want[case.name]).tobytes(), case


def test_every_ensemble_member_gets_its_own_constants():
    """The constants a recorder set uploads for a solver of five members (``ObserverSet._bind_inputs``).
    The check of a real Ensemble is tests/test_gpu_vocabulary.py's test of the same name; the host
    emulation has no observer kernels, so on the CPU the upload is caught at a stand-in handle.  Kept
    because it is the only CPU test that fails when every member is handed member 0's constants."""
    class Handle:
        solver = None
        consts = None

        def set_x(self, x):
            pass

        def set_consts(self, values):
            self.consts = np.array(values)

    class Solver:
        nsys, N = 5, vc.NARG
        class model:
            spec = dict(uses_x=0)

    model = vc.carrier_model()
    rs = recorders.RecorderSet(model, vc.NARG)
    for c in vc.HOSTC_GROUP:
        rs.add(c.name, c.expr)
    handle = Handle()
    bound = recorders._Bound(handle, rs._lower(0)[1])
    rs._bind = lambda solver: bound
    ks = np.array([0.8125, -0.3, 1.7, 2.0 ** -20, 3.25])
    rs._bind_inputs(Solver, vc.carrier_x(), [[k, 1.25] for k in ks])
    want = np.array([[np.exp(k), np.log(k + 2), k ** 3, np.float64(1.25) ** 3] for k in ks])
    assert handle.consts.tobytes() == want.tobytes()


# ---- probes ------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,periodic,P", [(1003, True, 31), (1003, False, 300), (257, True, 5)])
def test_probes_of_the_helpers(N, periodic, P):
    x, U = vc.probe_state(N, periodic)
    model = vc.carrier_model()
    exprs, kinds = [e for e, _ in vc.PROBE_CASES], [k for _, k in vc.PROBE_CASES]
    nodes, got = phost.run(model, exprs, kinds, x, dict(x=x, U=U, V=U + 1, W=U + 2), dict(k=0.75, c=1.25), periodic, P)
    disc = [vc.discretise(model, e) for e in exprs]
    inputs = [x, U, U + 1, U + 2, 0.75, 1.25, periodic]
    exact, ref = vc.exact_nodes(model, disc, inputs), vc.numpy_nodes(model, disc, inputs)
    dx = (x[-1] - x[0]) / (N - 1)
    for n, (expr, kind) in enumerate(vc.PROBE_CASES):
        if "tanh" not in expr:
            assert nodes[n].tobytes() == ref[n].tobytes(), expr
        f = np.array([float(v) for v in exact[n]])
        want = vc.reduce_exact(kind, f, x, dx, periodic)
        if kind in ("sum", "mean", "integral"):
            assert abs(got[n] - want) <= 1e-14 * vc.reduce_scale(kind, f, dx), (expr, kind, got[n], want)
        else:
            assert got[n] == want, (expr, kind, got[n], want)


# ---- models ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(vc.MODEL_CASES))
def test_model_cases(name, backend):
    for periodic in (True, False):
        for per_node in (False, True):
            vc.check_model_case(name, backend, periodic, per_node)


def test_the_model_cases_hold_the_whole_vocabulary():
    """F and J of the cases, between them: every construct the emitter lowers."""
    text = ""
    for name in vc.MODEL_CASES:
        m = vc.case_model(name, oracle=True)
        text += codegen.lower_model(m)[0] + codegen.lower_model(m, parvec_mask=(1 << len(m._pars)) - 1)[0]
    for token in ("sin(", "cos(", "tan(", "tanh(", "sinh(", "cosh(", "exp(", "log(", "atan(", "asin(", "acos(", "sqrt(",
                  "tf_sq(", "tf_powi(", "pow(", "tf_max(", "tf_min(", "tf_div_u(", "tf_hc[", "xc", "(1.0 / "):
        assert token in text, token
    for n in (3, 4, 5, 6, 7, 15, 16, -2):     # (SymPy prints c * u**-5 as c / u**5: tf_powi(u, 5) under a division)
        assert "tf_powi(v_U, %d)" % n in text or "tf_powi(v_V, %d)" % n in text or "tf_powi(v_W, %d)" % n in text, n
    m = vc.case_model("arith", oracle=True)                  # Heaviside from Max: identically one in J
    assert "Heaviside" in str(m._J_sparse_array) and "Heaviside" not in codegen.lower_model(m)[0]


# ---- refusals ----------------------------------------------------------------------------------
def _cache_listing():
    return sorted(os.listdir(compilers.CACHE_DIR)) if os.path.isdir(compilers.CACHE_DIR) else []


@pytest.mark.parametrize("args,match", [
    (("k * dxxU + erf(U)", "U", ["k"]), "erf"),
    (("k * dxxU + atan2(U, k)", "U", ["k"]), "arctan2"),
    (("k * dxxU + Piecewise((U, U > 0), (0, True))", "U", ["k"]), "select"),
    (("k * dxxU + Heaviside(U - 1) * U", "U", ["k"]), "DiracDelta"),
    ((["k * dxxxx%s" % v for v in "ABCDEFGHI"], list("ABCDEFGHI"), ["k"]), r"b = 2 x 9 = 18"),
])
def test_models_the_back_end_refuses(args, match):
    before = _cache_listing()
    with pytest.raises(UnsupportedExpression, match=match):
        Model(*args)
    assert _cache_listing() == before


@pytest.mark.parametrize("expr,match", vc.REFUSED)
def test_observers_the_back_end_refuses(expr, match):
    model = vc.carrier_model()
    x, U = vc.probe_state(50, True)
    sim = Simulation(model, dict(x=x, U=U, V=U, W=U), dict(k=1e-3, c=1.25, periodic=True), dt=1e-3, time_stepping=False)
    before = _cache_listing()
    with pytest.raises(UnsupportedExpression, match=match):
        sim.add_recorder("r", expr)
    with pytest.raises(UnsupportedExpression, match=match):
        sim.add_probe("p", expr, reduce="max")
    assert sim.recorders == {} and sim.probes == {} and sim._recorders.names == [] and sim._probes.names == []
    assert _cache_listing() == before
