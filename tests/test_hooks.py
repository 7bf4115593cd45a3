"""Expression hooks on the CPU: ``ExpressionHook.__call__`` and the kernels' walks (tests/hook_host: csrc/tf_hook.h
compiled with g++) against the hand-written Python functions of tests/hook_cases.py, bit for bit; what is
refused; the lowering and the code object."""
import re
import subprocess

import numpy as np
import pytest

from tests import hook_cases as hc
from tests.hook_host.build_hook_host import Harness
from triflow_amd import codegen, compilers, device, schemes
from triflow_amd.hooks import ExpressionHook

T = 0.37


def same(a, b):
    return np.asarray(a, dtype=float).tobytes() == np.asarray(b, dtype=float).tobytes()


def assert_state(got, want, names, what):
    for n in names:
        assert same(got[n], want[n]), "%s: %s differs at nodes %s" % (
            what, n, np.flatnonzero(np.asarray(got[n]).view(np.uint64) != np.asarray(want[n]).view(np.uint64))[:8])


def grids_of(name):
    return [N for N in hc.GRIDS if N >= hc.CASES[name][3]]


def test_exported_next_to_dirichlet_hook():
    assert schemes.ExpressionHook is ExpressionHook and device.ExpressionHook is ExpressionHook
    assert "ExpressionHook" in schemes.__all__


@pytest.mark.parametrize("name", sorted(hc.CASES))
@pytest.mark.parametrize("special", [False, True])
def test_call_equals_hand_written(name, special):
    """``hook(t, fields, pars)`` on host containers and on plain dicts of arrays."""
    for N in grids_of(name):
        mname, statements, _ = hc.case(name, N)
        model = hc.model(mname)
        hook = ExpressionHook(model, statements)
        before, want = hc.expected(name, N, T, special=special)
        pars = hc.pars_of(mname, N)
        fields = model.fields_template(**before)
        out, out_pars = hook(T, fields, pars)
        assert out is fields and out_pars is pars
        assert_state(out, want, model._dep_vars, "%s N=%d container" % (name, N))
        plain = {k: v.copy() for k, v in before.items()}
        hook(T, plain, pars)
        assert_state(plain, want, model._dep_vars, "%s N=%d dict" % (name, N))
        assert hook.launches(N) <= hc.LAUNCHES[name]
        if N >= 203:
            assert hook.launches(N) == hc.LAUNCHES[name]


@pytest.mark.parametrize("name", sorted(hc.CASES))
def test_harness_equals_hand_written(name):
    """The walks of tfk_hook_window / tfk_hook_points, thread by thread: every grid, periodic and clamped,
    one chunk, ragged chunks and chunks of length 1; plain states and states with NaN, infinities and zeros."""
    for N in grids_of(name):
        mname, statements, _ = hc.case(name, N)
        model = hc.model(mname)
        pars = hc.pars_of(mname, N)
        mask = 1 if mname == "helper" else 0
        x = hc.fields_of(mname, N)["x"]
        for P in hc.CHUNKS[N]:
            for periodic in ((False, True) if N < 4099 else (False,)):
                h = Harness(model, statements, x, pars, periodic, P, parvec_mask=mask)
                for special in (False, True):
                    before, want = hc.expected(name, N, T, special=special)
                    got = h.apply(T, before)
                    assert_state(got, want, model._dep_vars,
                                 "%s N=%d P=%d periodic=%s special=%s" % (name, N, P, periodic, special))


def test_swap_second_statement_sees_the_first():
    N = 203
    before, want = hc.expected("swap", N, T)
    assert want["U"][0] == before["U"][-1] and want["U"][-1] == before["U"][-1]      # as Python does


def test_clip_is_numpy_maximum():
    model = hc.model("scalar")
    hook = ExpressionHook(model, [("U", slice(None), "Max(U, 1e-6)")])
    x = np.linspace(0, 1, 7)
    U = np.array([-0.0, np.nan, -np.inf, np.inf, 0.0, 1e-7, 2.0])
    want = np.maximum(U, 1e-6)
    h = Harness(model, [("U", slice(None), "Max(U, 1e-6)")], x, hc.pars_of("scalar", 7), False, 3)
    assert same(h.apply(0.0, dict(x=x, U=U))["U"], want)
    f = dict(x=x, U=U.copy())
    hook(0.0, f, hc.pars_of("scalar", 7))
    assert same(f["U"], want)
    assert np.isnan(want[1]) and want[0] == 1e-6 and want[2] == 1e-6


REFUSED = [
    (("U", 0, "dxU"), "derivatives"),
    (("U", slice(None), "dxxU * k"), "derivatives"),
    (("U", 0, "upwind(c, U, 1)"), "upwind"),
    (("U", slice(None), "at(U, 0)"), "window"),
    (("U", 0, "Heaviside(U)"), "Heaviside"),
    (("U", 0, "U + nosuch"), "nosuch"),
    (("U", 0, "at(V, 0)"), "at"),
    (("U", 0, "at(U, k)"), "at"),
    (("V", 0, "1"), "dependent variable"),
    (("U", 1.5, "1"), "integer node or a slice"),
    (("U", slice(None, None, -1), "U"), "step >= 1"),
    (("U", slice(None, None, 0), "U"), ""),
]


@pytest.mark.parametrize("statement,word", REFUSED)
def test_refusals_name_the_statement(statement, word):
    good = ("U", 0, "1")
    with pytest.raises(ValueError) as err:
        ExpressionHook(hc.model("scalar"), [good, statement])
    assert "statement 1" in str(err.value) and word in str(err.value)


def test_exact_mode_takes_heaviside():
    ExpressionHook(hc.model("exact"), [("U", 0, "Heaviside(U - c)")])


def test_node_out_of_range_at_first_use():
    hook = ExpressionHook(hc.model("scalar"), [("U", 0, "1"), ("U", 300, "1")])
    assert hook.layout(301)[1].target == 300
    with pytest.raises(ValueError, match="statement 1"):
        hook.layout(203)
    hook = ExpressionHook(hc.model("scalar"), [("U", 0, "at(U, -300)")])
    with pytest.raises(ValueError, match="statement 0"):
        hook.layout(203)
    x = np.linspace(0, 1, 7)
    with pytest.raises(ValueError, match="statement 0"):
        hook(0.0, dict(x=x, U=x.copy()), hc.pars_of("scalar", 7))


def test_empty_window_is_legal():
    hook = ExpressionHook(hc.model("scalar"), [("U", slice(5, 5), "0"), ("U", slice(300, None), "0")])
    x = np.linspace(0, 1, 203)
    f = dict(x=x, U=x.copy())
    hook(0.0, f, hc.pars_of("scalar", 203))
    assert same(f["U"], x) and hook.launches(203) == 0


def test_idempotent_is_derived():
    film = hc.model("film")
    inlet = ExpressionHook(film, hc.case("film_inlet", 203)[1])
    assert inlet.idempotent and inlet.time_dependent
    assert not ExpressionHook(film, hc.case("film_open", 203)[1]).idempotent
    assert not ExpressionHook(film, [("h", 0, "1"), ("h", slice(-40, None), "h - k * (h - 1)")]).idempotent
    assert not ExpressionHook(film, [("h", -1, "at(h, -2)")]).idempotent
    const = ExpressionHook(film, [("h", slice(None), "1 + eps * x")])
    assert const.idempotent and not const.time_dependent


def test_parameters_callable_updates_pars():
    model = hc.model("scalar")
    hook = ExpressionHook(model, [("U", 0, "k")], parameters=lambda t, pars: dict(k=pars["k"] + t))
    x = np.linspace(0, 1, 7)
    f = dict(x=x, U=x.copy())
    _, pars = hook(2.0, f, dict(k=1.0, c=0.0))
    assert pars["k"] == 3.0 and f["U"][0] == 3.0


def test_lowering_one_case_per_statement_and_t_only_in_host_constants():
    model = hc.model("film")
    hook = ExpressionHook(model, hc.case("film_full", 203)[1] + [("T", 5, "T + t")])
    block, spec = hook.lowered(203)
    n = len(hook.statements)
    assert "#define TF_NHOOK %d" % n in block and "#define TF_NHOOK_HC 2" in block
    assert "#define TF_HOOK_USES_X 0" in block
    for k in range(n):
        assert len(re.findall(r"^    case %d: return " % k, block, flags=re.M)) == 1
    assert spec["host_consts"] == ["sin(2 * pi * c * t)", "t"]
    assert spec["runs"] == [(0, 5), (5, 3), (8, 1)]
    body = block[block.index("TF_DEVICE double tf_eval_hook"):]
    # t reaches the body as a host constant and as nothing else: no argument, no literal
    assert re.findall(r"\btf_t\b[^;\n]*;", body)[0] == "tf_t = tf_hc[1];"
    assert not re.search(r"\bt\b", body.replace("tf_t", ""))
    assert "static constexpr int tf_hook_kind[%d] = {0, 0, 0, 0, 0, 1, 1, 1, 0};" % n in block
    assert "static constexpr int tf_hook_at_node[4] = {201, 201, 200, 201};" in block
    v = codegen.eval_host_constants(spec, 0.1, [1.5, 0.25, 0.01, 0.0625], t=0.4)
    assert v == [float(np.sin(2 * np.pi * 1.5 * 0.4)), 0.4]


def test_code_object_of_kind_hook_holds_exactly_the_two_kernels():
    assert compilers._OBSERVER_SKELETON["hook"][-1] == "tf_hook.h"
    model = hc.model("scalar")
    block, _ = ExpressionHook(model, hc.case("scalar_open", 203)[1]).lowered(203)
    hsaco = compilers.build_observer_code_object(model, block, "hook")
    syms = subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-readelf", "-s", "-W", hsaco], capture_output=True, text=True,
                          check=True).stdout
    kernels = sorted(set(re.findall(r"FUNC\s+GLOBAL\s+\S+\s+\S+\s+(tfk_\w+)", syms)))
    assert kernels == ["tfk_hook_points", "tfk_hook_window"]
    usage = compilers.resource_usage(hsaco)
    assert sorted(usage) == kernels and all(u["ScratchSize"] == 0 for u in usage.values())
    with open(hsaco[:-len(".hsaco")] + ".json") as f:
        assert '"kind": "hook"' in f.read()


def test_other_model_is_refused_by_the_stepper():
    class FakeCompiled:
        model = hc.model("film")

    stepper = object.__new__(device.Stepper)
    stepper.compiled = FakeCompiled()
    with pytest.raises(ValueError, match="another model"):
        stepper.program(ExpressionHook(hc.model("scalar"), [("U", 0, "1")]))
