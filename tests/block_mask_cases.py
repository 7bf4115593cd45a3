"""Checks of the block mask of the banded solver, shared by the CPU emulation suite
(tests/test_block_mask.py) and the GPU suite (tests/test_gpu_block_mask.py).

A model whose variables are not fully coupled (the film model: h and q do not read T; the stiff
model: nothing reads E) has solver blocks with structurally zero entries -- the complement of the
reflexive-transitive closure of its Jacobian pattern (codegen.block_mask).  The level-1 kernels skip
them: no arithmetic, no stored planes.  The reference of every check is the same run with
TRIFLOW_BLOCK_MASK=0, where the generated header carries the all-true mask and the kernels are the
dense code, and the oracle (oracle/numpy_path.py, SuperLU):

  * each of the two runs lies within the model's STEP_TOL (tests/parity_cases.py) of the oracle,
  * the masked run is no further from the oracle than 4 x the dense run + 1e-15 (the skipped
    operations multiply exact zeros; where the dense pivot search would have taken a row of another
    class the results differ by rounding, which is what the factor 4 allows for),
  * where the pivots stay inside their class the two states are equal bit for bit.

Not checked here: that the planes of the masked-out entries are never written (there is no
test-side access to the stored factors, and none is added for it), and the rescue plan of
check_unstable_factorisation_recovers (a scalar model: its mask is full)."""
import os
from functools import partial

import numpy as np

from oracle import corpus, numpy_path as ora
from tests.parity_cases import STEP_TOL
from triflow_amd import Model, codegen
from triflow_amd.compilers import hip_compiler
from triflow_amd.device import DirichletHook
from triflow_amd.ensemble import Ensemble

#: the tolerance of "other" models in tests/parity_cases.py (cfg1, diff_per, burgers_per, ...)
OTHER_TOL = 1e-11


def with_env(pairs, fn):
    """fn() with the environment variables of ``pairs`` set."""
    old = {k: os.environ.get(k) for k in pairs}
    os.environ.update({k: str(v) for k, v in pairs.items()})
    try:
        return fn()
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def make_model(margs, backend):
    """(the mask is read when the model is lowered: a model object per setting of the switch)"""
    compiler = hip_compiler if backend is None else partial(hip_compiler, backend=backend)
    return Model(*margs, compiler=compiler)


# ------------------------------------------------------------------------------------------ mask contents
def closure_by_powers(nvar, pat_eq, pat_var):
    """(I + G)^(nvar - 1) > 0: the reflexive-transitive closure, as a boolean matrix power"""
    g = np.eye(nvar, dtype=np.int64)
    g[np.asarray(pat_eq, dtype=int), np.asarray(pat_var, dtype=int)] = 1
    p = np.eye(nvar, dtype=np.int64)
    for _ in range(max(nvar - 1, 1)):
        p = ((p @ g) > 0).astype(np.int64)
    return p > 0


MASK_MODELS = {"M3_film": 7, "M5_stiff": 21, "wave": 4, "tri3": 9}


def check_mask_contents(name):
    m = Model(*corpus.model_args(name), compiler=lambda m: (None, None))
    src, spec = with_env(dict(TRIFLOW_BLOCK_MASK="1"), lambda: codegen.lower_model(m))
    nvar = spec["nvar"]
    want = closure_by_powers(nvar, spec["pat_eq"], spec["pat_var"])
    got = np.array(spec["blk_nz"], dtype=bool)
    assert got.shape == (nvar, nvar) and np.array_equal(got, want), (name, got, want)
    assert int(got.sum()) == MASK_MODELS[name], (name, int(got.sum()))
    full = bool(got.all())
    assert ("#define TF_BLK_FULL %d" % full) in src
    rows = ", ".join("{%s}" % ", ".join("true" if v else "false" for v in row) for row in got)
    assert ("tf_blk_nz[%d][%d] = {%s};" % (nvar, nvar, rows)) in src, name
    # the switch: the all-true mask, another header (so another code object / emulation library)
    src0, spec0 = with_env(dict(TRIFLOW_BLOCK_MASK="0"), lambda: codegen.lower_model(m))
    assert np.array(spec0["blk_nz"], dtype=bool).all() and "#define TF_BLK_FULL 1" in src0
    assert (src0 == src) == full, name
    if name == "M3_film":
        h, q, T = 0, 1, 2                    # h and q do not read T
        assert not got[h, T] and not got[q, T] and got[T, h] and got[T, q]
    if name == "M5_stiff":
        assert not got[:4, 4].any() and got[4, :].all()          # nothing reads E


# ------------------------------------------------------------------------------------------ masked against dense
FILM_HOOK = dict(h={0: 1.0, -1: 1.0})
HOOKS = {None: (None, None),
         "cfg5": (DirichletHook(A={0: 1.0, -1: 1.0}), corpus.dirichlet_hook_cfg5),
         "film": (DirichletHook(**FILM_HOOK), None)}


def _film_hook(t, fields, pars):
    for node, value in FILM_HOOK["h"].items():
        fields["h"][node] = value
    return fields, pars


HOOKS["film"] = (HOOKS["film"][0], _film_hook)

ORACLE_SCHEMES = {"ROS2": lambda m: ora.ROS2(m), "RODASPR": lambda m: ora.RODASPR(m, time_stepping=False),
                  "BDF2": lambda m: ora.BDF2(m), "Theta": lambda m: ora.Theta(m)}


def member_inputs(case):
    """x, fields [nsys][N], parameters (one value per member for those in `vary`), dt"""
    if case["inputs"] == "config":
        name, fd, pars, dt, _ = corpus.config_inputs(case["cfg"], case["N"])
    else:
        name, N = case["model"], case["N"]
        fd = corpus.synthetic_fields(name, N, seed=7, periodic=case["periodic"], length=N * 5e-3)
        pars, dt = corpus.synthetic_pars(name, N, case["periodic"]), case["dt"]
    nsys = case.get("nsys", 1)
    pars = dict(pars, periodic=case["periodic"])
    fields = {k: np.repeat(v[None, :], nsys, axis=0) * (1 + 0.01 * np.arange(nsys))[:, None]
              for k, v in fd.items() if k != "x"}
    for key in case.get("vary", ()):
        pars[key] = pars[key] * (1.0 + 0.25 * np.arange(nsys))
    return name, fd["x"], fields, pars, dt


_ORACLE = {}


def oracle_state(case, margs=None):
    """[nvar][nsys][N] after the case's steps, computed once per case and shared (read only)."""
    key = case["id"]
    if key not in _ORACLE:
        name, x, fields, pars, dt = member_inputs(case)
        mo = Model(*(margs or corpus.model_args(name)), compiler=ora.numpy_compiler)
        nsys = case.get("nsys", 1)
        out = []
        for e in range(nsys):
            p = {k: (v[e] if np.ndim(v) == 1 and k in case.get("vary", ()) else v) for k, v in pars.items()}
            f = mo.fields_template(x=x, **{k: v[e] for k, v in fields.items()})
            scheme = ORACLE_SCHEMES[case["scheme"]](mo)
            kw = dict(hook=HOOKS[case.get("hook")][1]) if case.get("hook") else {}
            t = 0.0
            with np.errstate(all="ignore"):
                for _ in range(case["steps"]):
                    t, f = scheme(t, f, dt, p, **kw)
            out.append(np.array([np.asarray(f[v]) for v in mo._dep_vars]))
        ref = np.array(out).transpose(1, 0, 2).copy()
        ref.setflags(write=False)
        _ORACLE[key] = ref
    return _ORACLE[key]


def device_state(backend, case, mask, margs=None, **env):
    name, x, fields, pars, dt = member_inputs(case)

    def run():
        m = make_model(margs or corpus.model_args(name), backend)
        ens = Ensemble(m, x, fields, pars, bool(pars["periodic"]), scheme=case["scheme"],
                       hook=HOOKS[case.get("hook")][0], nstate=3, **case.get("opts", {}))
        for _ in range(case["steps"]):
            ens.step(dt)
        ens.sync()
        st = ens.state().copy()
        desc = ens.solver.describe()
        ens.close()
        return st, desc
    return with_env(dict(env, TRIFLOW_BLOCK_MASK=mask), run)


def check_masked_against_dense(backend, case, tol, margs=None, bit_equal=None, **env):
    """Returns (error of the masked run, error of the dense run) against the oracle."""
    ref = oracle_state(case, margs)
    masked, desc = device_state(backend, case, "1", margs, **env)
    dense, _ = device_state(backend, case, "0", margs, **env)
    assert masked.shape == ref.shape and np.isfinite(masked).all() and np.isfinite(dense).all(), case["id"]
    scale = np.abs(ref).max()
    e_mask, e_dense = np.abs(masked - ref).max() / scale, np.abs(dense - ref).max() / scale
    same = np.array_equal(masked, dense)
    print("block mask %-28s %s: masked %.2e dense %.2e (tol %.0e) bit-equal %s  [%s]"
          % (case["id"], env or "", e_mask, e_dense, tol, same, desc))
    assert e_dense <= tol, (case["id"], env, "dense", e_dense)
    assert e_mask <= tol, (case["id"], env, "masked", e_mask)
    assert e_mask <= 4 * e_dense + 1e-15, (case["id"], env, e_mask, e_dense)
    if bit_equal:
        assert same, (case["id"], env, np.abs(masked - dense).max())
    return e_mask, e_dense


def film_case(cid, N, periodic, nsys, scheme, hook=None, **opts):
    return dict(id=cid, inputs="config", cfg=3, N=N, periodic=periodic, nsys=nsys, scheme=scheme, steps=5,
                vary=("c", "We") if nsys > 1 else (), hook=hook, opts=opts)


def stiff_case(cid, N, nsys=1, **opts):
    return dict(id=cid, inputs="config", cfg=5, N=N, periodic=False, nsys=nsys, scheme="BDF2", steps=5,
                hook="cfg5", opts=opts)


FILM_TOL, STIFF_TOL = STEP_TOL["film_per"], STEP_TOL["stiff_clamp"]
assert STEP_TOL["film_clamp"] == FILM_TOL

#: CPU tier: N = 203 and 2100, clamped and periodic, 1 and 3 members, ROS2 and RODASPR
FILM_CASES_CPU = [film_case("film_%d_%s_%dm_%s" % (N, "per" if periodic else "clamp", nsys, sch), N, periodic, nsys, sch)
                  for N in (203, 2100) for periodic in (True, False) for nsys, sch in ((1, "ROS2"), (3, "RODASPR"),
                                                                                       (3, "ROS2"), (1, "RODASPR"))]

#: the film case from a synthetic initial state whose pivots stay inside their class
BIT_CASE = dict(id="film_203_synthetic", inputs="synthetic", model="M3_film", N=203, periodic=True, nsys=1,
                scheme="ROS2", steps=5, dt=1e-3, opts={})


def check_pivots_stay_in_class(case):
    """The pivot search of the dense code takes the largest entry of a column among the rows not yet used.
    It stays inside the class of the column when every entry of A = I - c J below the diagonal block of
    a class is smaller than the class's own pivot candidates.  For the film model (classes {h, q} and {T})
    that is: in the columns of h and q, the T row of every diagonal block is smaller in magnitude than
    the h / q entries the search compares it with.  The pivot blocks of the walk are Schur complements
    of these blocks, so this is the necessary condition on the inputs; the proof that the case
    qualifies is the bit equality it is used for."""
    name, x, fields, pars, dt = member_inputs(case)
    mo = Model(*corpus.model_args(name), compiler=ora.numpy_compiler)
    f = mo.fields_template(x=x, **{k: v[0] for k, v in fields.items()})
    J = mo.J(f, pars).toarray()
    nvar, N = 3, case["N"]
    gamma = 1.0 + 1.0 / np.sqrt(2.0)            # ROS2: c = gamma dt
    A = np.eye(nvar * N) - gamma * dt * J
    # unknown index of (variable v, node i): node-major or variable-major, whichever the oracle uses --
    # the one in which h and q do not read T
    for idx in (np.arange(nvar * N).reshape(N, nvar), np.arange(nvar * N).reshape(nvar, N).T):
        blocks = A[idx[:, :, None], idx[:, None, :]]         # [node][equation][variable]
        if np.abs(blocks[:, :2, 2]).max() == 0:
            break
    assert np.abs(blocks[:, :2, 2]).max() == 0 and np.abs(blocks[:, 2, :2]).max() > 0
    in_class = np.minimum(np.abs(blocks[:, 0, 0]), np.abs(blocks[:, 1, 1]))
    cross = np.maximum(np.abs(blocks[:, 2, 0]), np.abs(blocks[:, 2, 1]))
    assert (cross < 0.5 * in_class).all(), (cross.max(), in_class.min())


# ------------------------------------------------------------------------------------------ cross-class pivot
#: one-way coupling with a large entry below the diagonal block: the dense pivot search exchanges the
#: rows of A and B, the masked one keeps them (pivoting inside the classes {A} and {B})
CROSS_MODEL = (["k*dxxA - A", "k*dxxB + s*A*B"], ["A", "B"], ["k", "s"], None)
CROSS_CASE = dict(id="cross_class_pivot", N=203, periodic=True, nsys=1, scheme="Theta", steps=3, opts={})
CROSS_S, CROSS_K, CROSS_DT = 1e4, 1e-3, 1e-2


def cross_inputs():
    N = CROSS_CASE["N"]
    x = np.linspace(0, 10, N, endpoint=False)
    A = -(0.6 + 0.3 * np.cos(2 * np.pi * x / 10))            # negative: B decays, the matrix stays well conditioned
    B = 1.0 + 0.4 * np.sin(2 * np.pi * x / 10 * 3)
    return x, dict(A=A, B=B), dict(k=CROSS_K, s=CROSS_S, periodic=True), CROSS_DT


def check_cross_class_pivot(backend):
    x, fd, pars, dt = cross_inputs()
    mo = Model(*CROSS_MODEL, compiler=ora.numpy_compiler)
    # the row exchange happens: |A(B, A)| = c s |B| exceeds |A(A, A)| = 1 + c (2 k / dx^2 + 1) at every node
    dx = x[1] - x[0]
    assert (dt * CROSS_S * np.abs(fd["B"]) > 2 * (1 + dt * (2 * CROSS_K / dx ** 2 + 1))).all()
    scheme = ora.Theta(mo)
    f, t = mo.fields_template(x=x, **fd), 0.0
    for _ in range(CROSS_CASE["steps"]):
        t, f = scheme(t, f, dt, pars)
    ref = np.array([np.asarray(f[v]) for v in mo._dep_vars])[:, None, :]
    out = {}
    for mask in ("1", "0"):
        def run():
            m = make_model(CROSS_MODEL, backend)
            ens = Ensemble(m, x, {k: v[None, :] for k, v in fd.items()}, pars, True, scheme="Theta", nstate=3)
            assert np.array(ens.solver.model.spec["blk_nz"]).sum() == (3 if mask == "1" else 4)
            for _ in range(CROSS_CASE["steps"]):
                ens.step(dt)
            ens.sync()
            st = ens.state().copy()
            ens.close()
            return st
        out[mask] = with_env(dict(TRIFLOW_BLOCK_MASK=mask), run)
    scale = np.abs(ref).max()
    e_mask, e_dense = np.abs(out["1"] - ref).max() / scale, np.abs(out["0"] - ref).max() / scale
    print("block mask cross-class pivot: masked %.2e dense %.2e (tol %.0e)" % (e_mask, e_dense, OTHER_TOL))
    assert np.isfinite(out["1"]).all() and np.isfinite(out["0"]).all()
    assert e_dense <= OTHER_TOL and e_mask <= OTHER_TOL, (e_mask, e_dense)
