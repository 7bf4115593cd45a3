"""The function vocabulary of the generated code (codegen._CEmitter) against exact arithmetic: the case
table, the exact reference and the metrics that tests/test_vocabulary.py (CPU: the host builds of the same
generated code, glibc) and tests/test_gpu_vocabulary.py (MI355X: the HIP path, OCML) share.

Exact reference: the very SymPy objects the emitter lowers (``probes.discretise(...)``, ``model.F_array``,
``model._J_sparse_array``), printed by ``lambdify`` for mpmath and evaluated at ``PREC`` bits on the
ghost-padded views of ``oracle.numpy_path.stencil_views``; every input is converted exactly from its
double.  The expected values are computed at test time; nothing is stored.

Metrics: a function case is measured in ulps of the exact value; entry ``i`` of a model's F or J in
ulps of ``S_i``, the exact sum of the absolute values of the entry's top-level additive terms (a metric
that does not reward cancellation).

Bounds of the libm class: ``ceil(measured worst) + 1`` ulp per function, from the table of
profiles/r08_vocabulary.txt (device: OCML of ROCm on the MI355X; host: glibc), never above ``LIBM_CAP``.
"""
import math

import mpmath
import numpy as np
import sympy as sp
from mpmath import mp, mpf
from sympy import lambdify
from sympy.codegen import cfunctions as cf

from oracle import numpy_path as ora
from triflow_amd import probes

PREC = 240
#: what the project promises for a libm call of the generated code (a condition, not a measurement)
LIBM_CAP = 4

# ---------------------------------------------------------------------------------- exact reference


_MP_MODULES = [{"Heaviside": lambda *a: mpf(1)}, "mpmath"]


def discretise(model, expression):
    """``probes.discretise`` for a string; a SymPy expression over the model's symbolic arguments (the
    C99 functions SymPy has no string spelling for: ``sympy.codegen.cfunctions``) passes as it is."""
    if isinstance(expression, str):
        return probes.discretise(model, expression)
    return sp.sympify(expression)


def node_arguments(model, inputs):
    """Per symbolic argument of the model: the ghost-padded view ([N]) or the scalar."""
    env, N, _, _ = ora.stencil_views(model, *inputs)
    return [env[k] for k in model._args], N


def exact_terms(model, exprs, inputs):
    """For every expression, at every node: (exact value, exact sum of |top-level additive term|), as
    mpmath numbers at PREC bits.  Returns two lists [nexpr][N]."""
    args, N = node_arguments(model, inputs)
    terms = [list(sp.Add.make_args(sp.sympify(e))) for e in exprs]
    with mp.workprec(PREC):
        func = lambdify(model._symbolic_args, terms, modules=_MP_MODULES, cse=False)
        cols = [[mpf(float(v)) for v in a] if np.ndim(a) else mpf(float(a)) for a in args]
        values, sums = [[] for _ in exprs], [[] for _ in exprs]
        for i in range(N):
            out = func(*[c[i] if isinstance(c, list) else c for c in cols])
            for k, tl in enumerate(out):
                tl = [mpf(t) for t in tl]
                values[k].append(mpmath.fsum(tl))
                sums[k].append(mpmath.fsum(tl, absolute=True))
    return values, sums


def exact_nodes(model, exprs, inputs):
    return exact_terms(model, exprs, inputs)[0]


def numpy_nodes(model, exprs, inputs):
    """What NumPy computes from the same printed expressions (the reference's path), [nexpr][N]."""
    f = lambdify(model._symbolic_args, [sp.sympify(e) for e in exprs], modules=ora._lambdify_modules())
    args, N = node_arguments(model, inputs)
    with np.errstate(all="ignore"):
        vals = f(*args)
    return np.array([np.broadcast_to(np.asarray(v, dtype=float), (N,)) for v in vals])


def ulp_of(v):
    """The spacing of the doubles at the exact value ``v`` (mpf): 2**(e - 52), the subnormal spacing
    below the normal range."""
    if v == 0:
        return mpf(2) ** -1074
    e = mpmath.frexp(abs(v))[1] - 1
    return mpf(2) ** (max(int(e), -1022) - 52)


def ulp_errors(got, exact, scale=None):
    """|got - exact| / ulp(scale) per node (``scale``: the exact values themselves by default)."""
    scale = exact if scale is None else scale
    with mp.workprec(PREC):
        return np.array([float(abs(mpf(float(g)) - e) / ulp_of(s)) for g, e, s in zip(got, exact, scale)])


def not_nearest(got, exact):
    """Nodes where another double is closer to the exact value than ``got`` (the criterion of
    tests/test_math_helpers.py: correctly rounded <=> none)."""
    bad = []
    with mp.workprec(PREC):
        for i, (g, e) in enumerate(zip(got, exact)):
            err = abs(mpf(float(g)) - e)
            lo, hi = np.nextafter(g, -np.inf), np.nextafter(g, np.inf)
            if err > abs(mpf(float(lo)) - e) or err > abs(mpf(float(hi)) - e):
                bad.append(i)
    return bad


# ---------------------------------------------------------------------------------- argument sets
NARG = 3001          # nodes of a function case: ragged against every partition count used


def _fit(*parts):
    a = np.concatenate([np.ravel(np.asarray(p, dtype=float)) for p in parts])
    assert np.isfinite(a).all()
    return np.resize(a, NARG)


def _logu(rng, lo, hi, n, signs=True):
    v = 10.0 ** rng.uniform(lo, hi, n)
    return v * rng.choice([-1.0, 1.0], n) if signs else v


def _around(values, steps=(-2, -1, 0, 1, 2)):
    out = []
    for v in np.ravel(values):
        for s in steps:
            w = v
            for _ in range(abs(s)):
                w = np.nextafter(w, np.inf if s > 0 else -np.inf)
            out.append(w)
    return np.array(out)


def _trig(rng):
    m = np.concatenate([np.arange(-40, 41), rng.integers(-636619, 636619, 260)])    # |m pi/2| <= 1e6
    return _fit(rng.uniform(-20, 20, 700), _logu(rng, -300, 6, 500), rng.uniform(-1e6, 1e6, 96),
                _around(m * (np.pi / 2)))


def _exp(rng):
    return _fit(rng.uniform(-20, 20, 1500), rng.uniform(700, 709.78, 400), rng.uniform(-745.1, -700, 600),
                _logu(rng, -300, 0, 401), [709.782712893384, -745.13, 0.0, -0.0])


def _sinhcosh(rng):
    return _fit(rng.uniform(-20, 20, 1500), _logu(rng, -300, 0, 600), rng.uniform(700, 710.47, 450),
                -rng.uniform(700, 710.47, 449), [710.4758600739439, -710.4758600739439])


def _expm1(rng):
    return _fit(_logu(rng, -300, 1.5, 2000), rng.uniform(30, 709.78, 500), -rng.uniform(30, 1e3, 400),
                rng.uniform(-1, 1, 101))


def _log1p(rng):
    return _fit(_logu(rng, -300, 300, 1500, signs=False), -_logu(rng, -300, -0.01, 900, signs=False),
                -(1 - 2.0 ** -np.arange(1, 54)), rng.uniform(-0.5, 1, 548))


def _tanh(rng):
    return _fit(_logu(rng, -300, 1.4, 2200), rng.uniform(-1, 1, 600), rng.uniform(18, 25, 201))


def _atan(rng):
    return _fit(_logu(rng, -300, 300, 2200), rng.uniform(-3, 3, 801))


def _asin(rng):
    one = _around([1.0], (-8, -7, -6, -5, -4, -3, -2, -1, 0))
    return _fit(_logu(rng, -300, 0, 1500), rng.uniform(-1, 1, 1000), one, -one, 1 - 2.0 ** -np.arange(1, 53),
                -(1 - 2.0 ** -np.arange(1, 53)), rng.choice([-1.0, 1.0], 379))


def _acos(rng):
    one = _around([1.0], (-8, -7, -6, -5, -4, -3, -2, -1, 0))
    return _fit(rng.uniform(-1, 1, 2000), _logu(rng, -300, 0, 500), one, -one, 1 - 2.0 ** -np.arange(1, 53),
                -(1 - 2.0 ** -np.arange(1, 53)), rng.choice([-1.0, 1.0], 379))


def _log(rng):
    return _fit(_around([1.0], range(-40, 41)), 1 + _logu(rng, -16, -0.5, 600), _logu(rng, -300, 300, 1200, False),
                5e-324 * 2.0 ** rng.integers(0, 52, 300) * rng.uniform(1, 2, 300), [5e-324, 2.2250738585072014e-308],
                10.0 ** rng.uniform(300, 308.2, 300), rng.uniform(0.5, 2, 518))


def _sqrt(rng):
    return _fit([0.0, 5e-324, 2.2250738585072014e-308], 5e-324 * 2.0 ** rng.integers(0, 52, 500) *
                rng.uniform(1, 2, 500), _logu(rng, -300, 300, 1500, False), rng.uniform(0, 4, 998))


def _pos(rng):
    return _fit(_logu(rng, -100, 100, 2000, False), rng.uniform(0.05, 3, 1001))


def _round(rng):
    n = rng.integers(-1000, 1000, 500).astype(float)
    big = np.concatenate([2.0 ** rng.integers(52, 200, 200) * rng.uniform(1, 2, 200), [2.0 ** 52, 2.0 ** 53]])
    return _fit([0.0, -0.0], n, n + 0.5, _around(n), big, -big, 2.0 ** 52 - 0.5 - np.arange(8), _logu(rng, -300, 0, 400),
                rng.uniform(-50, 50, 1000))


def _signs(rng):
    return _fit(np.tile([0.0, -0.0], 40), _logu(rng, -300, 300, 1500), [5e-324, -5e-324], rng.uniform(-2, 2, 1419))


def _small_ints(rng, n=NARG):
    """Many ties; zeros of both signs."""
    return rng.choice([-2.0, -1.0, -0.0, 0.0, 1.0, 2.5, 1e-300, -1e300], n)


def _zeros_both_orders():
    """(U, V, W) that open with (+0, -0, +0), (-0, +0, -0), ..."""
    return (np.tile([0.0, -0.0], 8), np.tile([-0.0, 0.0], 8), np.tile([0.0, 0.0, -0.0, -0.0], 4))


def _powi_base(rng):
    return _fit(rng.uniform(0.05, 3, 1600), -rng.uniform(0.05, 3, 600), _logu(rng, -15, 15, 700),
                [1e-4, 2.5e-7, 1 / 3, 100 / 999999, 1.0, -1.0], rng.uniform(0.9, 1.1, 95))


def all_ones(rng, n):
    """Doubles whose significand is all ones (the documented exception of tf_div_u), over many binades."""
    return np.ldexp(2.0 - 2.0 ** -52, rng.integers(-300, 300, n)) * rng.choice([-1.0, 1.0], n)


def is_all_ones(d):
    m, _ = np.frexp(np.abs(d))
    return m == 1.0 - 2.0 ** -53


# ---------------------------------------------------------------------------------- function cases
#: the carrier of the function cases: a recorder with pool="sample" over every node returns the raw
#: per-node value of its expression; U, V, W are the arguments, k and c scalars or per-node arrays
CARRIER = (["k * dxxU", "k * dxxV", "k * dxxW"], ["U", "V", "W"], ["k", "c"])
_U = sp.Symbol("U")


class FunctionCase:
    """One expression ``f(g(u))`` and its argument set.

    kind: "op" (one IEEE operation: bytes of NumPy, <= 0.5 ulp), "exact" (IEEE operations and FMAs only:
    bytes of NumPy), "powi" (correctly rounded power), "npowi" (reciprocal power: <= 1 ulp), "divu" (quotients
    over a hoisted divisor), "libm" (a libm call: the measured bound of ``fn``), "hostc" (a host constant)."""

    def __init__(self, name, expr, kind, args, fn=None, k=0.75, c=1.25, n=None, exact=None):
        # (k: a scalar, or a function of the generator for a per-node array; exact: u -> the exact value,
        # where the printed expression is not what SymPy's mpmath printer evaluates)
        self.name, self.expr, self.kind, self.fn, self.n, self.exact = name, expr, kind, fn or name, n, exact
        self._args, self.k, self.c = args, k, c

    def state(self):
        """dict(U, V, W, k, c): [NARG] arrays (k, c: scalars unless the case sets an array)."""
        rng = np.random.default_rng(sum(map(ord, self.name)))
        got = self._args(rng)
        got = got if isinstance(got, tuple) else (got,)
        fields = [np.resize(np.asarray(a, dtype=float), NARG) for a in got]
        while len(fields) < 3:
            fields.append(rng.uniform(0.5, 2.0, NARG))
        k = self.k(rng) if callable(self.k) else self.k
        return dict(U=fields[0], V=fields[1], W=fields[2], k=k, c=self.c)

    @property
    def per_node(self):
        return callable(self.k)

    def __repr__(self):
        return self.name


def carrier_x(periodic=True):
    return np.linspace(0.5, 30.0, NARG, endpoint=not periodic)


def carrier_inputs(state, periodic=True):
    """The positional inputs of the carrier (x, U, V, W, k, c, periodic)."""
    return [carrier_x(periodic), state["U"], state["V"], state["W"], state["k"], state["c"], periodic]


def _maxmin_args(rng):
    z = _zeros_both_orders()
    return tuple(np.concatenate([zi, _small_ints(rng, NARG - 16)]) for zi in z)


def _divu_args(rng):
    """U, W over V: V over 200 binades, the first 200 of them with an all-ones significand."""
    v = _logu(rng, -100, 100, NARG)
    v[:200] = all_ones(rng, 200)
    return _logu(rng, -100, 100, NARG), v, _logu(rng, -100, 100, NARG)


def _knode(lo, hi):
    return lambda rng: rng.uniform(lo, hi, NARG)


LIBM_GROUP = [FunctionCase(n, "%s(U)" % n, "libm", a) for n, a in (
    ("sin", _trig), ("cos", _trig), ("tan", _trig), ("exp", _exp), ("sinh", _sinhcosh), ("cosh", _sinhcosh),
    ("tanh", _tanh), ("atan", _atan), ("asin", _asin), ("acos", _acos), ("log", _log))] + [
    # (SymPy has no string spelling for these four; its NumPy printer prints numpy.log2 ... for the objects)
    FunctionCase("log2", cf.log2(_U), "libm", _log), FunctionCase("log10", cf.log10(_U), "libm", _log),
    FunctionCase("log1p", cf.log1p(_U), "libm", _log1p), FunctionCase("expm1", cf.expm1(_U), "libm", _expm1),
    FunctionCase("sin(x)*u", "sin(x) * U", "libm", lambda rng: _logu(rng, -100, 100, NARG)),
]

EXACT_GROUP = [
    FunctionCase("sqrt", "sqrt(U)", "op", _sqrt),
    FunctionCase("u**0.5", "U**0.5", "op", _sqrt),
    FunctionCase("u**-1", "U**-1", "op", lambda rng: _logu(rng, -300, 300, NARG)),
    FunctionCase("u**2", "U**2", "op", lambda rng: _logu(rng, -150, 150, NARG)),
    FunctionCase("abs", "Abs(U)", "op", _signs),
    FunctionCase("sign", "sign(U)", "op", _signs),
    FunctionCase("floor", "floor(U)", "op", _round),
    FunctionCase("ceil", "ceiling(U)", "op", _round),
    FunctionCase("max2", "Max(U, V)", "op", _maxmin_args),
    FunctionCase("min2", "Min(U, V)", "op", _maxmin_args),
    FunctionCase("max3", "Max(U, V, W)", "exact", _maxmin_args),
    FunctionCase("min3", "Min(U, V, W)", "exact", _maxmin_args),
    FunctionCase("u/k", "U / k", "op", lambda rng: _logu(rng, -100, 100, NARG), k=0.3),
    FunctionCase("u/x", "U / x", "op", lambda rng: _logu(rng, -100, 100, NARG)),
    # two quotients over one node-dependent divisor: one true division for the reciprocal, tf_div_u twice
    FunctionCase("u/v", "U / V", "divu", _divu_args),
    FunctionCase("w/v", "W / V", "divu", _divu_args),
    FunctionCase("shared", "dxU / (1 + U**2) + U / (1 + U**2)", "exact", lambda rng: _logu(rng, -3, 100, NARG)),
]
POWI_GROUP = [FunctionCase("u**%d" % n, "U**%d" % n, "powi", _powi_base, n=n) for n in range(3, 17)]
NPOWI_GROUP = [FunctionCase("u**%d" % n, "U**(%d)" % n, "npowi", _powi_base, n=n) for n in range(-2, -17, -1)]
#: pow with a constant / node-dependent exponent, and the uniform sub-expressions with a per-node k
#: (k per node: exp(k) ... are calls of the device libm)
POW_GROUP = [
    FunctionCase("u**1.5", "U**1.5", "libm", _pos, fn="pow", k=_knode(0.5, 1.5)),
    FunctionCase("u**-0.5", "U**-0.5", "libm", _pos, fn="pow", k=_knode(0.5, 1.5)),
    # (SymPy: U**(1/3), printed and lowered as pow(u, 1.0 / 3.0), NaN for u < 0, as NumPy evaluates it; the
    # yardstick is the power with that rounded exponent -- 38 ulp from the cube root at u = 1e99)
    FunctionCase("cbrt", "cbrt(U)", "libm", _pos, fn="pow", k=_knode(0.5, 1.5), exact=lambda u: u ** mpf(1.0 / 3.0)),
    FunctionCase("2**u", "2**U", "libm", lambda rng: _fit(rng.uniform(-1070, 1023, 2000), rng.uniform(-3, 3, 1001)),
                 fn="pow", k=_knode(0.5, 1.5)),
    FunctionCase("u**u", "U**U", "libm", lambda rng: _fit(10.0 ** rng.uniform(-3, 2.1, 2000), rng.uniform(0.5, 3, 1001)),
                 fn="pow", k=_knode(0.5, 1.5)),
    FunctionCase("u**k", "U**k", "libm", lambda rng: 10.0 ** rng.uniform(-2, 2, NARG), fn="pow", k=_knode(-30, 30)),
    FunctionCase("exp(k) per node", "exp(k)", "libm", _pos, fn="exp", k=_knode(-20, 20)),
    # (the rounding of k + 2 is part of this figure: a row of its own in the table)
    FunctionCase("log(k+2) per node", "log(k + 2)", "libm", _pos, fn="log(k+2)", k=_knode(0, 50)),
    FunctionCase("k**3 per node", "k**3", "powi", _pos, k=_knode(-3, 3), n=3),
]
#: the same three with a scalar k: evaluated on the host with NumPy, handed over as extra scalars
HOSTC_GROUP = [FunctionCase("exp(k)", "exp(k)", "hostc", _pos, k=0.8125 + 2.0 ** -40),
               FunctionCase("log(k+2)", "log(k + 2)", "hostc", _pos, k=0.8125 + 2.0 ** -40),
               FunctionCase("k**3", "k**3", "hostc", _pos, k=0.8125 + 2.0 ** -40),
               FunctionCase("dxu*exp(k)+u*c**3", "dxU * exp(k) + U * c**3", "hostc", _pos, k=0.8125 + 2.0 ** -40)]

#: name -> (cases of one recorder set, parameter-vector mask of the carrier: bit 0 = k per node)
FUNCTION_GROUPS = {"libm": (LIBM_GROUP, 0), "exact": (EXACT_GROUP, 0), "powi": (POWI_GROUP, 0),
                   "npowi": (NPOWI_GROUP, 0), "pow": (POW_GROUP, 1), "hostc": (HOSTC_GROUP, 0)}

# ---------------------------------------------------------------------------------- libm bounds
#: worst error in ulp measured against mpmath on the argument sets above (profiles/r08_vocabulary.txt):
#: (MI355X, OCML of the ROCm the table names; host build, glibc).  ``bound`` below is the rule of the
#: suite: ceil(measured) + 1, and never above LIBM_CAP.
MEASURED_ULP = {
    "sin": (0.690, 0.504), "cos": (0.669, 0.561), "tan": (0.762, 0.682), "exp": (0.794, 0.501),
    "sinh": (0.546, 1.590), "cosh": (0.529, 1.604), "tanh": (0.841, 1.827), "atan": (1.253, 0.499),
    "asin": (0.621, 0.501), "acos": (0.706, 0.503), "log": (0.581, 0.500), "log2": (0.601, 0.506),
    "log10": (0.590, 1.382), "log1p": (0.602, 0.744), "expm1": (0.881, 0.731), "pow": (1.222, 0.503),
    # composites: the rounding of k + 2 / of the product is part of the figure
    "log(k+2)": (1.377, 1.377), "sin(x)*u": (1.240, 1.181),
}


def libm_bound(fn, device):
    measured = MEASURED_ULP[fn][0 if device else 1]
    bound = math.ceil(measured) + 1
    assert bound <= LIBM_CAP, (fn, measured)
    return bound



# ---------------------------------------------------------------------------------- probe cases
#: (expression, reduction): the natural observers of the helpers a model equation cannot hold (SymPy
#: cannot print their derivatives for J)
PROBE_CASES = [("Abs(dxU)", "sum"), ("sign(U - 1)", "mean"), ("Max(U, 1)", "max"), ("floor(3 * U)", "argmax"),
               ("tanh(U)", "integral")]


def probe_state(N, periodic):
    rng = np.random.default_rng(N)
    x = np.linspace(0.0, 4.0, N, endpoint=not periodic)
    U = 1.0 + np.sin(2 * np.pi * x / 4.0 * 3) + 0.3 * rng.standard_normal(N)
    U[::97] = 1.0                       # sign(U - 1) = 0 there
    return x, U


def reduce_exact(kind, f, x, dx, periodic):
    """The reduction of the exact node values rounded to double (``f``), as tests/test_probes.py has it."""
    if kind == "sum":
        return math.fsum(f)
    if kind == "mean":
        return math.fsum(f) / f.size
    if kind == "integral":
        return dx * math.fsum(f) if periodic else dx * (math.fsum(f) - (f[0] + f[-1]) / 2)
    if kind in ("argmax", "argmin"):
        return x[getattr(np, kind)(f)]
    return getattr(np, kind)(f)


def reduce_scale(kind, f, dx):
    return math.fsum(np.abs(f)) * {"integral": dx, "mean": 1.0 / f.size}.get(kind, 1.0)


#: (expression, what the refusal names): what the emitter has no lowering for, and a Heaviside of the
#: user's own (identically one in J, where it is the derivative of Max / Min; an observer has no J)
REFUSED = [("erf(U)", "erf"), ("atan2(U, V)", "arctan2"), ("Piecewise((U, U > 0), (0, True))", "select"),
           ("Heaviside(U - 1) * U", "Heaviside")]


# ---------------------------------------------------------------------------------- model cases
#: name -> (equations, dependent variables, parameters, help functions, arithmetic only).  Every equation
#: is k * dxxU + <term>; between them F and the SymPy-derived J hold every construct the emitter lowers
#: (J brings 1/sqrt, u**(n-1), 1/cosh**2, Heaviside == 1 from Max).  Arithmetic only: + - * / sqrt, squares,
#: reciprocals, Max/Min -- bit-identical to the NumPy oracle.
def _three(*terms):
    return (["k * dxx%s + %s" % (v, t.replace("@", v)) for v, t in zip("UVW", terms)], list("UVW")[:len(terms)])


MODEL_CASES = {
    "arith": (*_three("@ * dx@ / (1 + @**2) + @ / (1 + @**2)", "sqrt(1 + @) / (c + @)", "Max(@, 1) * dx@ + Min(@, c)**2"),
              ["k", "c"], None, True),
    "arith_x": (*_three("@ / x + dx@**2", "c / (x + @)", "Max(@, x / 2, 1) * @"), ["k", "c"], None, True),
    "trig": (*_three("sin(@)", "cos(c * @)", "tan(@ / 2)"), ["k", "c"], None, False),
    "hyper": (*_three("tanh(@)", "sinh(@) * dx@", "cosh(@ - c)"), ["k", "c"], None, False),
    "explog": (*_three("exp(-@)", "log(1 + @**2)", "exp(c) * @ + log(c + 2) * dx@"), ["k", "c"], None, False),
    "inverse": (*_three("atan(@)", "asin(@ / 4)", "acos(@ / 4)"), ["k", "c"], None, False),
    "powi": (*_three("@**3 + c**3 * @", "@**7", "@**16"), ["k", "c"], None, False),
    "npowi": (*_three("@**-2", "c * @**-5", "dx@ * @**-3"), ["k", "c"], None, False),
    "pow": (*_three("@**1.5", "@**-0.5", "2**@"), ["k", "c"], None, False),
    "powvar": (*_three("@**@", "@**c", "sqrt(@) * @**0.25"), ["k", "c"], None, False),
    "mixed_x": (*_three("sin(x) * @", "exp(-x) * dx@", "Max(@, 1)**3"), ["k", "c"], None, False),
    "two_var": (["k * dxxU + sin(V) * U - U**3", "c * dxxV - U * exp(-V) + dxU * tanh(V)"], ["U", "V"], ["k", "c"],
                None, False),
    "helper_fn": (["k * dxxU + tanh(s) * U + sqrt(s) * dxU + c * dxs"], ["U"], ["k", "c"], ["s"], False),
}
MODEL_N = 301        # ragged against the partitions of the solver


def model_inputs(name, periodic, per_node, N=MODEL_N):
    """(fields dict with x, parameter dict): smooth positive fields in (0.3, 2.9) with noise (asin(u / 4),
    u**u, sqrt(1 + u) are defined), scalar or per-node k and c."""
    eqs, dep, pars, helps, _ = MODEL_CASES[name]
    rng = np.random.default_rng(sum(map(ord, name)) + 2 * periodic + per_node)
    x = np.linspace(0.25, 3.25, N, endpoint=not periodic)
    fields = dict(x=x)
    for j, v in enumerate(list(dep) + list(helps or [])):
        fields[v] = 1.6 + np.cos(2 * np.pi * (x - 0.25) / 3.0 * (j + 1) + j) + 0.25 * rng.uniform(-1, 1, N)
    if per_node:
        p = dict(k=1e-3 * (1 + 0.5 * np.sin(2 * np.pi * x / 3.0)), c=1.3 + 0.4 * rng.uniform(-1, 1, N))
    else:
        p = dict(k=1e-3, c=1.3 + 2.0 ** -30)
    return fields, p


# ---------------------------------------------------------------------------------- the host build
# (the generated record block of a function group compiled with g++ by tests/observer_host: the CPU tier
# measures it, the GPU tier compares the bytes of its exact-class rows with the device's)
_CARRIER_MODEL = []
_HOST_GROUPS = {}


def carrier_model():
    from triflow_amd import Model
    if not _CARRIER_MODEL:
        _CARRIER_MODEL.append(Model(*CARRIER, hold_compilation=True))
    return _CARRIER_MODEL[0]


def group_expressions(gname):
    model = carrier_model()
    return [discretise(model, c.expr) for c in FUNCTION_GROUPS[gname][0]]


def host_group(gname):
    """(ctypes library, record spec, generated block) of a function group, built once per process."""
    import os
    from tests.observer_host import common
    from tests.record_host import build_record_host as rhost
    from triflow_amd import codegen
    if gname not in _HOST_GROUPS:
        mask = FUNCTION_GROUPS[gname][1]
        block, spec = codegen.lower_records(carrier_model(), group_expressions(gname), parvec_mask=mask)
        lib = common.build(carrier_model(), block, os.path.join(rhost.HERE, "record_host.cpp"), rhost.HEADERS, mask)
        _HOST_GROUPS[gname] = (lib, spec, block)
    return _HOST_GROUPS[gname]


def host_row(gname, case, periodic=True, P=31):
    """The per-node values [NARG] of ``case`` from the host build of its group."""
    from tests.observer_host import common
    cases, mask = FUNCTION_GROUPS[gname]
    lib, spec, _ = host_group(gname)
    st = case.state()
    fields = {v: st[v] for v in "UVW"}
    x = carrier_x(periodic)
    L, arrays = common.system_planes(carrier_model(), spec, x, fields, dict(k=st["k"], c=st["c"]), periodic, P, mask)
    out = np.zeros(NARG)
    lib.record_host_run(common.C.byref(L), *[common.dptr(a) for a in arrays], cases.index(case), 0, 0, NARG, 1,
                        common.dptr(out))
    return out


def case_references(gname, case, periodic=True):
    """(exact node values as mpmath numbers, NumPy's values) of a function case."""
    model = carrier_model()
    disc = [discretise(model, case.expr)]
    inputs = carrier_inputs(case.state(), periodic)
    if case.exact is not None:
        with mp.workprec(PREC):
            exact = [case.exact(mpf(float(u))) for u in inputs[1]]
    else:
        exact = exact_nodes(model, disc, inputs)[0]
    return exact, numpy_nodes(model, disc, inputs)[0]


# ---------------------------------------------------------------------------------- running a model case
_MODELS = {}
_LIBM_TOKENS = {"pow", "tf_powi", "exp", "log", "sin", "cos", "tan", "tanh", "sinh", "cosh", "atan", "asin", "acos",
                "log10", "log2", "cbrt", "expm1", "log1p"}


def case_model(name, backend=None, oracle=False):
    """The model of a case: HIP path (``backend=None``), a test back end, or uncompiled (``oracle``)."""
    from functools import partial
    from triflow_amd import Model
    from triflow_amd.compilers import hip_compiler
    key = (name, id(backend), oracle)
    if key not in _MODELS:
        eqs, dep, pars, helps, _ = MODEL_CASES[name]
        if oracle:
            _MODELS[key] = Model(eqs, dep, pars, helps, hold_compilation=True)
        else:
            compiler = hip_compiler if backend is None else partial(hip_compiler, backend=backend)
            _MODELS[key] = Model(eqs, dep, pars, helps, compiler=compiler)
    return _MODELS[key]


def is_arithmetic_only(model, parvec_mask=0):
    """No pow / libm call in the generated F and J (host constants are NumPy's own values)."""
    from triflow_amd import codegen
    src, _ = codegen.lower_model(model, parvec_mask=parvec_mask)
    return not (codegen._tokens(src) & _LIBM_TOKENS)


def device_FJ(name, backend, periodic, per_node):
    """F [nvar][N] and the raw Jacobian value table [nnz][N] of a model case from the kernels."""
    m = case_model(name, backend)
    fd, p = model_inputs(name, periodic, per_node)
    cm = m._device
    values = [p[k] for k in cm.pars]
    N = fd["x"].size
    solver = cm.solver(N, periodic, 1, cm.parvec_mask_of(values))
    cm.bind_inputs(solver, fd["x"], values, [fd[k] for k in m._help_funcs] if cm.nh else None)
    solver.set_state(0, np.array([fd[k] for k in m._dep_vars]))
    solver.eval(0, with_j=True)
    F = np.array(solver.get_F()[0]).reshape(N, m._nvar).T
    J = np.array(solver.get_J()[0]).reshape(N, -1).T
    return F, J


def model_references(name, periodic, per_node):
    """Per F row / J entry: exact values, exact S, and the NumPy oracle's values ([rows][N] each)."""
    m = case_model(name, oracle=True)
    fd, p = model_inputs(name, periodic, per_node)
    inputs = [fd["x"]] + [fd[k] for k in list(m._dep_vars) + list(m._help_funcs)] + [p[k] for k in m._pars] + [periodic]
    out = []
    for exprs in (m.F_array.tolist(), m._J_sparse_array.tolist()):
        values, sums = exact_terms(m, exprs, inputs)
        out.append((values, sums, numpy_nodes(m, exprs, inputs)))
    return out


def s_scaled_worst(got, values, sums):
    """Worst |got - exact| / ulp(S) over the rows and nodes."""
    return max(ulp_errors(g, v, s).max() for g, v, s in zip(got, values, sums))


def check_model_case(name, backend, periodic, per_node, report=None):
    """The assertions of a model case (both tiers); ``report``: a list that receives the figures
    (tools/gpu_vocabulary_table.py writes them into the profile)."""
    m = case_model(name, oracle=True)
    F, J = device_FJ(name, backend, periodic, per_node)
    (fv, fs, fnp), (jv, js, jnp) = model_references(name, periodic, per_node)
    tag = "%s %s %s" % (name, "periodic" if periodic else "clamped", "per-node" if per_node else "scalar")
    mask = (1 << len(m._pars)) - 1 if per_node else 0
    arithmetic = MODEL_CASES[name][4]
    assert arithmetic == is_arithmetic_only(m, mask), tag
    figures = dict(case=tag, F_dev=s_scaled_worst(F, fv, fs), F_numpy=s_scaled_worst(fnp, fv, fs),
                   J_dev=s_scaled_worst(J, jv, js), J_numpy=s_scaled_worst(jnp, jv, js))
    print("%(case)-32s F: kernel %(F_dev).3f NumPy %(F_numpy).3f   J: kernel %(J_dev).3f NumPy %(J_numpy).3f  ulp(S)"
          % figures)
    if report is not None:
        report.append(figures)
    if arithmetic:
        assert np.array_equal(F, fnp), tag
        assert (np.abs(J - jnp) <= 2 * np.spacing(np.abs(jnp))).all(), tag
    else:
        # the device's libm cap over NumPy's roughly one ulp; never asked to go below 2 ulp(S)
        assert figures["F_dev"] <= max(4 * figures["F_numpy"], 2.0), figures
        assert figures["J_dev"] <= max(4 * figures["J_numpy"], 2.0), figures
