"""TEST-ONLY: the cases of the expression hooks (triflow_amd/hooks.py) and, for each, the hand-written
Python function that is the yardstick: the statements executed in the order given on NumPy arrays, each
right-hand side evaluated completely before its assignment.

A case is a model, a list of statements (a function of the number of nodes ``N`` where a target is placed
relative to it), the parameters and ``reference(t, f, p)``, which assigns into the dict of arrays ``f``.  The
references are written as a user would write the hook, operand order as SymPy prints the statement (the
contract of a value is the lambdified expression).  No non-square integer power of a node value appears
(NumPy's vectorised ``pow`` is one ulp off the correctly rounded power of the kernels).
"""
import numpy as np

from triflow_amd import Model
from triflow_amd.workloads import model_args

GRIDS = (7, 203, 4099)
#: chunk counts of the host harness per grid: one chunk, ragged chunks (N % P != 0), chunks of length 1
CHUNKS = {7: (1, 3, 7), 203: (1, 8, 64), 4099: (128,)}

_MODELS = {}


def model(name, compiled=False):
    """The models of the cases: ``scalar`` (k * dxxU - c * dxU), ``film`` (three variables), ``helper`` (a help
    function ``s`` and the parameter ``k`` given per node) and ``exact`` (Heaviside in the exact mode)."""
    key = (name, compiled)
    if key not in _MODELS:
        kw = dict(hold_compilation=not compiled)
        if name == "scalar":
            _MODELS[key] = Model(*model_args("M1_advdiff"), **kw)
        elif name == "film":
            _MODELS[key] = Model(*model_args("M3_film"), **kw)
        elif name == "helper":
            _MODELS[key] = Model(["k * dxxU + s"], "U", "k", "s", **kw)
        elif name == "exact":
            _MODELS[key] = Model("k*dxxU - Heaviside(c)*dxU", "U", ["k", "c"], heaviside="exact", **kw)
        else:
            raise KeyError(name)
    return _MODELS[key]


def pars_of(name, N):
    if name == "scalar":
        return dict(k=0.125, c=0.75)
    if name == "film":
        return dict(c=1.5, eps=0.25, We=0.01, k=0.0625)
    if name == "helper":
        return dict(k=0.5 + 0.25 * np.cos(np.arange(N) * 0.7))          # per node
    return dict(k=0.125, c=0.3)


def fields_of(name, N, seed=0, special=False):
    """x and the fields of model ``name`` on ``N`` nodes, deterministic.  ``special``: NaN, the infinities and
    both zeros placed in the state (first, last and interior nodes among them)."""
    rng = np.random.RandomState(1000 * seed + N)
    x = np.linspace(0.0, 10.0, N)
    names = {"scalar": ["U"], "film": ["h", "q", "T"], "helper": ["U", "s"], "exact": ["U"]}[name]
    f = {"x": x}
    for j, n in enumerate(names):
        f[n] = 1.0 + 0.5 * np.sin(x * (j + 1)) + 0.1 * rng.standard_normal(N)
    if special:
        vals = [np.nan, np.inf, -np.inf, -0.0, 0.0, 1e-7, -1e-300]
        for n in names:
            if n == "s":
                continue
            pos = rng.permutation(N)[:len(vals)]
            f[n][pos] = vals[:pos.size]
            f[n][0], f[n][-1] = -0.0, np.nan
            rng.shuffle(vals)
    return f


# ---- the hand-written references -------------------------------------------------------------------
def _ref_scalar_open(t, f, p):
    U, k, c = f["U"], p["k"], p["c"]
    U[0] = 1 + k * np.sin(2 * np.pi * c * t)
    U[-1] = U[-2]
    U[-40:] = U[-40:] - k * (U[-40:] - 1)
    U[:] = np.maximum(U, 0.25)


def _ref_swap(t, f, p):
    U = f["U"]
    U[0] = U[-1]
    U[-1] = U[0]


def _ref_order(t, f, p):
    U, x = f["U"], f["x"]
    U[3] = 2 * U[3]
    U[2:6] = U[2:6] + 1                    # reads what the point statement wrote
    U[4] = U[4] * U[4]                     # reads what the window statement wrote
    U[0::3] = U[0::3] * 0.5
    U[:] = U + x                           # second statement of the run reads the first's target


def _ref_windows(N):
    mid = N // 2

    def ref(t, f, p):
        U, k, c = f["U"], p["k"], p["c"]
        U[5:6] = U[5:6] + 10
        U[3:3] = 0.0
        U[1::3] = U[1::3] * c
        U[2:-1] = U[2:-1] - k
        U[mid] = U[mid] + t
        U[0] = U[mid] * c                 # at() across chunks
        U[-1] = U[1] + U[-2]
        U[1:2] = U[1:2] - k
    return ref


def _ref_film_inlet(t, f, p):
    f["h"][0] = 1 + p["eps"] * np.sin(2 * np.pi * p["c"] * t)


def _ref_film_open(t, f, p):
    h, q, T, k = f["h"], f["q"], f["T"], p["k"]
    h[0] = 1 + p["eps"] * np.sin(2 * np.pi * p["c"] * t)
    q[0] = 0.5 * (h[0] * h[0])
    h[-1] = h[-2]
    q[-1] = 2 * q[-2] - q[-3]
    T[-1] = T[-2]
    h[-40:] = h[-40:] - k * (h[-40:] - 1)
    q[-40:] = q[-40:] - k * (q[-40:] - 0.5 * (h[-40:] * h[-40:]))


def _ref_film_full(t, f, p):
    _ref_film_open(t, f, p)
    f["h"][:] = np.maximum(f["h"], 1e-6)


def _ref_helper(t, f, p):
    U, s, k = f["U"], f["s"], p["k"]
    U[:] = U + k * s
    U[0] = s[0] + k[0]
    U[-1] = s[0] + U[1]


def _ref_exact(t, f, p):
    U, x = f["U"], f["x"]
    U[:] = U * np.heaviside(U - p["c"], 0.5)
    U[:] = U + p["k"] * x


_FILM_OPEN = [
    ("h", 0, "1 + eps * sin(2 * pi * c * t)"),
    ("q", 0, "h * h * 0.5"),
    ("h", -1, "at(h, -2)"),
    ("q", -1, "2 * at(q, -2) - at(q, -3)"),
    ("T", -1, "at(T, -2)"),
    ("h", slice(-40, None), "h - k * (h - 1)"),
    ("q", slice(-40, None), "q - k * (q - h * h * 0.5)"),
]

#: name -> (model, statements(N), reference(N), smallest grid)
CASES = {
    "scalar_open": ("scalar", lambda N: [
        ("U", 0, "1 + k * sin(2 * pi * c * t)"), ("U", -1, "at(U, -2)"),
        ("U", slice(-40, None), "U - k * (U - 1)"), ("U", slice(None), "Max(U, 0.25)")],
        lambda N: _ref_scalar_open, 7),
    "swap": ("scalar", lambda N: [("U", 0, "at(U, -1)"), ("U", -1, "at(U, 0)")], lambda N: _ref_swap, 7),
    "order": ("scalar", lambda N: [
        ("U", 3, "2 * U"), ("U", slice(2, 6), "U + 1"), ("U", 4, "U * U"),
        ("U", slice(0, None, 3), "U * 0.5"), ("U", slice(None), "U + x")], lambda N: _ref_order, 7),
    "windows": ("scalar", lambda N: [
        ("U", slice(5, 6), "U + 10"), ("U", slice(3, 3), "0"), ("U", slice(1, None, 3), "U * c"),
        ("U", slice(2, -1), "U - k"), ("U", N // 2, "U + t"), ("U", 0, "at(U, %d) * c" % (N // 2)),
        ("U", -1, "at(U, 1) + at(U, -2)"), ("U", slice(1, 2), "U - k")], _ref_windows, 7),
    "film_inlet": ("film", lambda N: _FILM_OPEN[:1], lambda N: _ref_film_inlet, 7),
    "film_open": ("film", lambda N: list(_FILM_OPEN), lambda N: _ref_film_open, 7),
    "film_full": ("film", lambda N: _FILM_OPEN + [("h", slice(None), "Max(h, 1e-6)")],
                  lambda N: _ref_film_full, 7),
    "helper": ("helper", lambda N: [
        ("U", slice(None), "U + k * s"), ("U", 0, "s + k"), ("U", -1, "at(s, 0) + at(U, 1)")],
        lambda N: _ref_helper, 7),
    "exact": ("exact", lambda N: [
        ("U", slice(None), "U * Heaviside(U - c)"), ("U", slice(None), "U + x * k")], lambda N: _ref_exact, 7),
}

#: launches of one application: the maximal runs of consecutive statements of one kind
LAUNCHES = {"scalar_open": 2, "swap": 1, "order": 4, "windows": 3, "film_inlet": 1, "film_open": 2,
            "film_full": 2, "helper": 2, "exact": 1}


def case(name, N):
    """(model name, statements, reference) of case ``name`` on ``N`` nodes."""
    mname, statements, reference, _ = CASES[name]
    return mname, statements(N), reference(N)


def expected(name, N, t, seed=0, special=False, pars=None):
    """(input fields, fields after the hand-written function at ``t``): dicts of arrays."""
    mname, _, reference = case(name, N)
    before = fields_of(mname, N, seed, special)
    after = {k: v.copy() for k, v in before.items()}
    with np.errstate(all="ignore"):
        reference(t, after, pars_of(mname, N) if pars is None else pars)
    return before, after
