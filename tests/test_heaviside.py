"""The exact mode of Heaviside / DiracDelta / Piecewise on the CPU: the generated
text, the emulation back end (tests/emu: the generated source and csrc/tf_math.h compiled with g++) and
the record harness against ``lambdify`` with ``numpy.heaviside``; the default mode is untouched."""
import ast
import os
import pickle
from functools import partial

import numpy as np
import pytest
import sympy

from oracle import corpus
from tests import heaviside_cases as hc
from tests import vocab_cases as vc
from tests.emu import build_emu
from tests.record_host import build_record_host as rhost
from triflow_amd import Model, codegen, compilers, probes
from triflow_amd.codegen import UnsupportedExpression
from triflow_amd.compilers import hip_compiler
from triflow_amd.simulation import Simulation


@pytest.fixture(scope="module")
def backend():
    # -O0: half the compile time, and the same IEEE arithmetic (tests/test_vocabulary.py)
    return build_emu.EmuBackend(opt="-O0")


def _cache_listing():
    return sorted(os.listdir(compilers.CACHE_DIR)) if os.path.isdir(compilers.CACHE_DIR) else []


def _held(eqs, dep, pars, helps=None, **kw):
    return Model(eqs, dep, pars, helps, hold_compilation=True, **kw)


# ---- 1. the default mode is untouched -----------------------------------------------------------
def _existing_models():
    for name in sorted(corpus.MODELS_ALL):
        yield name, corpus.model_args(name)
    for name in sorted(vc.MODEL_CASES):
        eqs, dep, pars, helps, _ = vc.MODEL_CASES[name]
        yield name, (eqs, dep, pars, helps)


@pytest.mark.parametrize("name,args", list(_existing_models()), ids=[n for n, _ in _existing_models()])
def test_default_mode_lowers_the_same_source(name, args):
    absent, one = _held(*args), _held(*args, heaviside="one")
    for mask in (0, (1 << len(absent._pars)) - 1):
        src = codegen.lower_model(absent, parvec_mask=mask)[0]
        assert src == codegen.lower_model(one, parvec_mask=mask)[0]
        assert "tf_heaviside" not in src and "tf_select" not in src and "tf_div_x" not in src


def test_unknown_mode_is_a_value_error():
    with pytest.raises(ValueError, match="bogus"):
        _held(*hc.MODELS["burgers_up"], heaviside="bogus")
    with pytest.raises(ValueError, match="bogus"):
        hip_compiler(hc.model("burgers_up", "one", oracle=True), heaviside="bogus")


@pytest.mark.parametrize("name,match", [("pw", "select"), ("gate", "DiracDelta")])
def test_default_mode_still_refuses_and_points_to_the_opt_in(name, match):
    before = _cache_listing()
    for kw in ({}, dict(heaviside="one")):
        with pytest.raises(UnsupportedExpression, match=match) as err:
            Model(*hc.MODELS[name], **kw)
        assert 'heaviside="exact"' in str(err.value)
        assert str(err.value).startswith("function %r is not supported by the HIP compiler" % match)
    assert _cache_listing() == before


# ---- 2. F and J, bit for bit ---------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(hc.MODELS))
def test_F_and_J_equal_numpy_bit_for_bit(name, backend):
    for N in hc.MODEL_GRIDS:
        for periodic in (True, False):
            for per_node in (False, True):
                hc.check_FJ(name, backend, N, periodic, per_node)


def test_the_helper_at_its_four_cases(backend):
    """np.heaviside(a, h0) for a < 0, a > 0, a = +-0 and NaN, h0 from the printed call."""
    m = Model("k*dxxU + Heaviside(U, 0.25) + 2*Heaviside(-U) + 4*Heaviside(U - 1, 1)", "U", ["k"],
              compiler=partial(hip_compiler, backend=backend), heaviside="exact")
    x = np.linspace(0.0, 1.0, 20)
    U = np.array([0.0, -0.0, 1.0, -1.0, 5e-324, -5e-324, 2.0, 0.5, 1.0, 0.0, 0.25, 0.25, np.nan, 0.25, 0.25, np.inf,
                  0.25, 0.25, -np.inf, 0.25])
    pars = dict(k=0.0, periodic=False)
    F, J = hc.device_FJ(m, dict(x=x, U=U), pars)
    Fn, Jn = hc.numpy_FJ(m, dict(x=x, U=U), pars)
    assert hc.same_bits(F, Fn) and hc.same_bits(J, Jn)
    assert F[0][0] == 0.25 + 2 * 0.5 and F[0][3] == 2.0 and F[0][2] == 1.0 + 4.0 and np.isnan(F[0][12])


# ---- 3. J is the derivative of F -----------------------------------------------------------------
def test_J_is_the_derivative_of_F_only_in_exact_mode(backend):
    fields, pars = hc.order_state()
    U, eps = fields["U"], 1e-6
    assert np.abs(U).min() > 1e-3                 # no node within eps of a kink
    figures = {}
    for mode in ("exact", "one"):
        m = hc.model("burgers_up", mode, backend)
        J = np.asarray(m.J(m.fields_template(**fields), pars).todense())
        fd = np.zeros_like(J)
        fmax = 0.0
        for i in range(U.size):
            up, dn = U.copy(), U.copy()
            up[i] += eps
            dn[i] -= eps
            Fp = m.F(m.fields_template(x=fields["x"], U=up), pars)
            Fm = m.F(m.fields_template(x=fields["x"], U=dn), pars)
            fd[:, i] = (Fp - Fm) / (2 * eps)
            fmax = max(fmax, np.abs(Fp).max(), np.abs(Fm).max())
        figures[mode] = (np.abs(J - fd).max(), np.abs(J).max(), fmax)
        print("%s: max|J - central difference| = %.3e = %.3e max|J|" % (mode, figures[mode][0],
                                                                      figures[mode][0] / figures[mode][1]))
    err, jmax, fmax = figures["exact"]
    # F is piecewise quadratic: a central difference has no truncation error, only F's rounding
    assert err <= 64 * 2.0 ** -53 * fmax / eps, figures
    err, jmax, _ = figures["one"]
    assert err > 1e-3 * jmax, figures


# ---- 4. the step gains an order ------------------------------------------------------------------
def test_the_linearised_step_is_third_order_only_in_exact_mode(backend):
    hc.check_step_order(backend)


# ---- 5. observers --------------------------------------------------------------------------------
OBS_EXPRS = [hc.OBS_RIGHT, hc.OBS_PIECE, hc.OBS_STEP]


@pytest.mark.parametrize("per_node", [False, True], ids=["scalar", "per-node"])
def test_observer_node_values_equal_numpy_bit_for_bit(per_node):
    """The block every observer kernel evaluates, through the record harness (csrc/tf_record.h with g++)."""
    m = hc.observer_model("exact", compiled=False)
    for N, P in ((50, 3), (1031, 7), (2053, 5)):
        for periodic in (True, False):
            fields, pars, _ = hc.observer_inputs(N, periodic, per_node)
            fields["U"][30], fields["U"][33], fields["U"][36] = np.nan, np.inf, -np.inf
            mask = 2 if per_node else 0
            h = rhost.Harness(m, OBS_EXPRS, fields["x"], dict(U=fields["U"]), pars, periodic, P, mask)
            want = hc.numpy_nodes(m, OBS_EXPRS, fields, pars)
            for which in range(len(OBS_EXPRS)):
                got = h.row(which, "sample", slice(None))
                assert hc.same_bits(got, want[which]), (N, periodic, OBS_EXPRS[which])
            assert set(np.unique(want[0][~np.isnan(want[0])])) == {0.0, 0.5, 1.0}


@pytest.mark.parametrize("N,P", [(50, 3), (1031, 7), (2053, 5)])
@pytest.mark.parametrize("per_node", [False, True], ids=["scalar", "per-node"])
def test_the_five_observers_through_their_host_harnesses_over_three_steps(N, P, per_node, backend):
    """An integral probe of Heaviside(U), a recorder of a Piecewise, a mean statistic, a spectrum and the
    extrema of Heaviside(U - c) * U on the states of three emulated ROS2 steps."""
    for periodic in (True, False):
        states, pars = hc.stepped_states(backend, N, periodic, per_node)
        hc.check_observers_on_the_host(states, pars, periodic, P, per_node)


def test_every_observer_lowers_the_exact_vocabulary():
    m = hc.observer_model("exact", compiled=False)
    disc = [probes.discretise(m, e) for e in OBS_EXPRS]
    blocks = [codegen.lower_probes(m, disc, ["integral", "sum", "mean"])[0]] + \
        [lower(m, disc)[0] for lower in (codegen.lower_records, codegen.lower_statistics, codegen.lower_spectra,
                                         codegen.lower_extrema)]
    for block in blocks:
        assert "tf_heaviside(v_U, (1.0 / 2.0))" in block and "tf_heaviside((v_U - v_c), (1.0 / 2.0))" in block
        assert "tf_select((v_U > 0.0), v_U, tf_select(true, 0.0, tf_nan()))" in block


def test_observers_of_a_default_mode_model_refuse(backend):
    m = hc.observer_model("one", compiled=False)
    fields, pars, dt = hc.observer_inputs(50, True, False)
    sim = Simulation(m, fields, pars, dt=dt, time_stepping=False)
    before = _cache_listing()
    calls = [lambda e: sim.add_probe("p", e, reduce="integral"), lambda e: sim.add_recorder("r", e),
             lambda e: sim.add_statistic("s", e, stat="mean"), lambda e: sim.add_spectrum("f", e, modes=[0, 1]),
             lambda e: sim.add_extrema("x", e)]
    for expr, match in ((hc.OBS_RIGHT, "Heaviside"), (hc.OBS_STEP, "Heaviside"), (hc.OBS_PIECE, "select")):
        for call in calls:
            with pytest.raises(UnsupportedExpression, match=match) as err:
                call(expr)
            assert 'heaviside="exact"' in str(err.value)
    assert sim.probes == {} and sim.recorders == {} and sim.statistics == {} and sim.spectra == {} \
        and sim.extrema == {}
    assert _cache_listing() == before


# ---- 6. plane analyses ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["burgers_up", "gate", "pw"])
def test_discontinuous_entries_are_never_aliases(name):
    m = hc.model(name, "exact", oracle=True)
    for mask in (0, (1 << len(m._pars)) - 1):
        spec = codegen.lower_model(m, parvec_mask=mask)[1]
        marked = [k for k, e in enumerate(m._J_sparse_array.tolist())
                  if sympy.sympify(e).has(sympy.Heaviside, sympy.DiracDelta, sympy.Piecewise)]
        assert marked, name
        for k in marked:
            assert spec["j_alias"][k] < 0 and k not in spec["j_alias"], (name, k, spec["j_alias"])
    if name == "burgers_up":
        # (the default mode does alias entries of this model: the analysis is the mode's)
        one = codegen.lower_model(hc.model(name, "one", oracle=True))[1]
        print("default-mode aliases of burgers_up:", one["j_alias"])


@pytest.mark.parametrize("mode", ["one", "exact"])
def test_upwind_with_a_scalar_velocity_stays_constant_coefficient(mode):
    m = _held("k*dxxU - upwind(c, U, 1)", "U", ["k", "c"], heaviside=mode)
    spec = codegen.lower_model(m)[1]
    assert spec["j_uniform"] == [1] * spec["nnz"] and spec["uses_x"] == 0


def test_a_uniform_heaviside_is_evaluated_on_the_device():
    m = _held("k*dxxU - Heaviside(c)*dxU", "U", ["k", "c"], heaviside="exact")
    src, spec = codegen.lower_model(m)
    assert spec["j_uniform"] == [1] * spec["nnz"]
    uniform = src[src.index("TF_DEVICE void tf_eval_J_uniform"):]
    assert uniform.count("tf_heaviside(v_c, (1.0 / 2.0))") == 2
    assert not any("Heaviside" in h for h in spec["host_consts"]), spec["host_consts"]
    # with x or a per-node parameter in it, it is node-dependent
    assert codegen.lower_model(m, parvec_mask=2)[1]["j_uniform"] == [0, 1, 0]
    mx = _held("k*dxxU - Heaviside(x - 0.5)*dxU", "U", ["k"], heaviside="exact")
    assert codegen.lower_model(mx)[1]["uses_x"] == 1 and codegen.lower_model(mx)[1]["j_uniform"] == [0, 1, 0]


def test_uniform_planes_follow_the_sign_of_a_scalar_parameter(backend):
    hc.check_uniform_planes_follow_a_scalar(backend)


def test_a_hoisted_call_of_a_uniform_heaviside_has_numpys_bits(backend):
    """exp(Heaviside(c)) is a host constant: evaluated with NumPy, by the exact meaning of the name."""
    m = Model("k*dxxU + exp(Heaviside(c)) * U + exp(Piecewise((c, c > 0), (2 * c, True))) * U", "U", ["k", "c"],
              compiler=partial(hip_compiler, backend=backend), heaviside="exact")
    spec = codegen.lower_model(m)[1]
    assert any("Heaviside" in h for h in spec["host_consts"]) and any("select" in h for h in spec["host_consts"])
    x = np.linspace(0.0, 1.0, 20)
    U = 1.0 + np.cos(7 * x)
    for c in (-0.75, 0.0, -0.0, 1.5):
        pars = dict(k=1e-3, c=c, periodic=False)
        F, J = hc.device_FJ(m, dict(x=x, U=U), pars)
        Fn, Jn = hc.numpy_FJ(m, dict(x=x, U=U), pars)
        assert hc.same_bits(F, Fn) and hc.same_bits(J, Jn), c


def test_a_default_mode_host_constant_takes_heaviside_as_one(backend):
    """exp(Heaviside(c)) in the default mode: the hoisted constant is evaluated with the mode's meaning of
    the name, one, as the same Heaviside is in the kernels (before the modes it could not be evaluated)."""
    m = Model("k*dxxU + exp(Heaviside(c)) * U", "U", ["k", "c"], compiler=partial(hip_compiler, backend=backend))
    assert any("Heaviside" in h for h in codegen.lower_model(m)[1]["host_consts"])
    x = np.linspace(0.0, 1.0, 20)
    U = 1.0 + np.cos(7 * x)
    one = [{"Heaviside": lambda *a: 1}, "numpy"]
    for c in (-0.75, 0.0, 1.5):
        pars = dict(k=1e-3, c=c, periodic=False)
        F, _ = hc.device_FJ(m, dict(x=x, U=U), pars)
        assert hc.same_bits(F, hc.numpy_rows(m, m.F_array.tolist(), dict(x=x, U=U), pars, modules=one)), c


# ---- 7. persistence and cache --------------------------------------------------------------------
def test_pickle_and_save_keep_the_mode(tmp_path):
    m = _held(*hc.MODELS["burgers_up"], heaviside="exact")
    again = pickle.loads(pickle.dumps(m))
    assert again._heaviside == "exact" and codegen.lower_model(again)[0] == codegen.lower_model(m)[0]
    m.save(tmp_path / "burgers")
    assert Model.load(tmp_path / "burgers")._heaviside == "exact"
    assert pickle.loads(pickle.dumps(_held(*hc.MODELS["burgers_up"])))._heaviside == "one"
    # a pickle from before the keyword: six arguments
    from triflow_amd.model import _rebuild_model
    old = _rebuild_model(m._diff_eqs, m._dep_vars, m._pars, m._help_funcs, m._bdcs, "hip")
    assert old._heaviside == "one"


def test_the_two_modes_have_cache_entries_of_their_own():
    src_e, tag_e, _ = compilers.code_object_source(hc.model("burgers_up", "exact", oracle=True))
    src_o, tag_o, _ = compilers.code_object_source(hc.model("burgers_up", "one", oracle=True))
    assert tag_e != tag_o and "tf_heaviside" in src_e and "tf_heaviside" not in src_o
    # ... also where no expression differs
    heat = [compilers.code_object_source(_held("k*dxxU", "U", ["k"], heaviside=mode))[1] for mode in ("one", "exact")]
    assert heat[0] != heat[1]


def test_a_foreign_model_opts_in_through_the_compiler():
    keyword = codegen.lower_model(hc.model("burgers_up", "exact", oracle=True))[0]
    foreign = _held(*hc.MODELS["burgers_up"])
    del foreign._heaviside                        # as the reference's own Model class: no such attribute
    assert codegen.heaviside_mode(foreign) == "one"
    default = codegen.lower_model(foreign)[0]
    F, J = partial(hip_compiler, heaviside="exact")(foreign)
    assert codegen.lower_model(foreign)[0] == keyword != default
    assert F.device_model.model is foreign


def test_the_compiler_keyword_does_not_change_the_mode_of_a_model_that_has_one():
    with pytest.raises(ValueError, match="built with heaviside='one'"):
        Model(*hc.MODELS["burgers_up"], heaviside="one", compiler=partial(hip_compiler, heaviside="exact"))
    foreign = _held(*hc.MODELS["burgers_up"])
    del foreign._heaviside
    partial(hip_compiler, heaviside="exact")(foreign)
    partial(hip_compiler, heaviside="exact")(foreign)              # the same mode again: fine
    with pytest.raises(ValueError, match="built with heaviside='exact'"):
        hip_compiler(foreign, heaviside="one")
    assert foreign._heaviside == "exact"


# ---- 8. refusals in exact mode -------------------------------------------------------------------
@pytest.mark.parametrize("args,match", [
    (("k * dxxU + erf(U)", "U", ["k"]), "erf"),
    (("k * dxxU + atan2(U, k)", "U", ["k"]), "arctan2"),
])
def test_models_the_exact_mode_refuses(args, match):
    before = _cache_listing()
    with pytest.raises(UnsupportedExpression, match=match):
        Model(*args, heaviside="exact")
    assert _cache_listing() == before


@pytest.mark.parametrize("text", ["U * greater(U, 0)", "logical_and.reduce((greater(U, 0),less(U, 1)))",
                                  "logical_not(greater(U, 0))", "select([U], [U], default=nan)",
                                  "select([greater(U, 0)], [U, 1], default=nan)", "U > 0"])
def test_a_relational_is_a_condition_not_a_value(text):
    """The parser of the model's language lets no relational through as a value; whatever the printer
    would make of one, the emitter refuses it."""
    before = _cache_listing()
    for mode in ("exact", "one"):
        emit = codegen._CEmitter({"U": "v_U"}, (), mode)
        with pytest.raises(UnsupportedExpression):
            emit.visit(ast.parse(text, mode="eval").body)
    assert _cache_listing() == before


def test_default_mode_refuses_the_condition_functions_with_the_text_it_always_had():
    for text, name in (("U * greater(U, 0)", "greater"), ("logical_not(greater(U, 0))", "logical_not"),
                       ("logical_and.reduce((greater(U, 0),less(U, 1)))", "logical_and")):
        with pytest.raises(UnsupportedExpression, match="function %r is not supported by the HIP compiler$" % name):
            codegen._CEmitter({"U": "v_U"}, (), "one").visit(ast.parse(text, mode="eval").body)


def test_an_ITE_condition_is_lowered_as_the_And_Or_sympy_prints_for_it():
    """SymPy rewrites ITE(a, b, c) into And / Or before the NumPy printer sees it, so the condition arrives
    in the supported form: the lowering is that of the same condition spelled out."""
    ite = _held("k*dxxU + Piecewise((U, ITE(U > 0, U > 1, U < -1)), (0, True))", "U", ["k"], heaviside="exact")
    src = codegen.lower_model(ite)[0]
    src = src[src.index("TF_DEVICE void tf_eval_F"):]
    printed = str(codegen._printed_expressions(ite._symbolic_args, ite.F_array.tolist(), "exact")[0])
    assert "ITE" not in src and "tf_select(" in src and (" & " in src or " | " in src)
    fields, pars = hc.order_state()
    U = fields["U"] * 2.0
    want = hc.numpy_rows(ite, ite.F_array.tolist(), dict(x=fields["x"], U=U), pars)[0]
    inner = np.where(U > 0, U > 1, U < -1)
    assert np.array_equal(np.isnan(want), np.zeros(U.size, bool)) and inner.any() and not inner.all(), printed
    with pytest.raises(UnsupportedExpression, match="select"):
        Model("k*dxxU + Piecewise((U, ITE(U > 0, U > 1, U < -1)), (0, True))", "U", ["k"])
