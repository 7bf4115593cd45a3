"""Checks of the wide memory phases of the cyclic-reduction factorisation (csrc/tf_cr3_hip.h, TF_CR_WIDE_IO;
the index mapping is csrc/tf_cr_io.h), used by tests/test_gpu_cr_wide_io.py.

Only data movement differs between the two builds -- how a chunk's records come into LDS, how a node's
record and the chunk's share of the next level leave -- so every stored quantity, and with it every state
and every solution, is the same BIT FOR BIT as with -DTF_CR_WIDE_IO=0 (the loops of the parent kernel).
That is the check; each run is also held against the oracle with the bound the parity suite uses for
the model (tests/parity_cases.py STEP_TOL for the stepping models; for the linear solves the bounds of
check_linear_solve and of its callers in tests/test_gpu_parity.py: 1e-9, and 1e-7 for wide4, whose fourth
derivatives at dx = 5e-3 give cond(A) ~ 1e9 for both solvers).

The shapes are the smallest that reach every branch of the three phases: 4-node chunks on level 1
(TRIFLOW_M1=4 / m1=4) turn N = 2100 into 525 separators = 33 chunks (the last of 13 nodes) -> 3 -> 1 and the
folded top block; N = 203 with the default plan is 50 separators = 4 chunks (the last of 2 nodes) -> one ragged
chunk of 4 nodes; the clamped cases zero the
blocks beyond the ends of a system; b = 5 (stiff) and b = 3 (tri3) have the 16-byte pair that holds the
last entry of L and the first of D; b = 8 (wide4) is the one-copy lane layout.  The 256-thread form of the
kernel is chosen by the runtime above 1024 chunks, which no small grid reaches: it is forced
(TRIFLOW_CR_FACTOR_BLOCK=256) in one case, next to the N = 40 000 case with the default plan."""
import numpy as np
import scipy.sparse as sps
import scipy.sparse.linalg as spla

from oracle import corpus
from tests import block_mask_cases as bc
from tests import parity_cases as pc
from triflow_amd import compilers

NARROW = "-DTF_CR_WIDE_IO=0"
STEPS = 3


def _film(cid, N, periodic, nsys, **env):
    case = bc.film_case(cid, N, periodic, nsys, "ROS2", hook=None if periodic else "film")
    return dict(case, steps=STEPS), bc.FILM_TOL, env


def _stiff(cid, N, **env):
    return dict(bc.stiff_case(cid, N), steps=STEPS), bc.STIFF_TOL, env


DEEP = dict(TRIFLOW_M1="4")
STEP_CASES = [
    _film("wio_film_2100_per_1m", 2100, True, 1, **DEEP),
    _film("wio_film_2100_per_3m", 2100, True, 3, **DEEP),
    _film("wio_film_2100_clamp_hook_1m", 2100, False, 1, **DEEP),
    _film("wio_film_2100_clamp_hook_3m", 2100, False, 3, **DEEP),
    _film("wio_film_203_per_1m", 203, True, 1),
    _film("wio_film_203_clamp_hook_1m", 203, False, 1),
    _stiff("wio_stiff_2100_bdf2", 2100, **DEEP),
    _film("wio_film_2100_per_unfused", 2100, True, 1, TRIFLOW_L1CR_FUSE="0", **DEEP),
    _film("wio_film_2100_per_3m_block256", 2100, True, 3, TRIFLOW_CR_FACTOR_BLOCK="256", **DEEP),
    _film("wio_film_40000_per_3m", 40000, True, 3),
]


def _state(case, env, narrow):
    def run():
        return bc.device_state(None, case, "1", **env)
    if narrow:
        with compilers.extra_flags(NARROW):
            return run()
    return run()


def check_steps(case, tol, env):
    """States after STEPS steps: wide == narrow bit for bit, both within ``tol`` of the oracle."""
    ref = bc.oracle_state(case)
    wide, desc = _state(case, env, False)
    narrow, desc0 = _state(case, env, True)
    assert desc == desc0, (desc, desc0)
    scale = np.abs(ref).max()
    e_wide, e_narrow = np.abs(wide - ref).max() / scale, np.abs(narrow - ref).max() / scale
    same = np.array_equal(wide.view(np.uint64), narrow.view(np.uint64))
    print("cr wide io %-32s %s: wide %.2e narrow %.2e (tol %.0e) bit-equal %s  [%s]"
          % (case["id"], env, e_wide, e_narrow, tol, same, desc))
    assert wide.shape == ref.shape and np.isfinite(wide).all() and np.isfinite(narrow).all(), case["id"]
    assert e_narrow <= tol and e_wide <= tol, (case["id"], e_wide, e_narrow)
    assert same, (case["id"], np.abs(wide - narrow).max())


#: (model, N, solver options, bound against SuperLU)
SOLVE_CASES = [
    ("M3_film", 2100, dict(refine=0, m1=4), 1e-9),
    ("M5_stiff", 2100, dict(refine=0, m1=4), 1e-9),
    ("tri3", 203, dict(refine=0, m1=4), 1e-9),
    ("tri3", 2100, dict(refine=0, m1=4), 1e-9),
    ("wide4", 203, dict(refine=0, m1=4), 1e-7),
    ("wide4", 203, dict(refine=0), 1e-7),
]


def check_solve(name, N, opts, tol, c=0.01):
    """One factorisation + one solve of (I - cJ) x = b, periodic and clamped, refinement off: wide == narrow
    bit for bit, both within ``tol`` of SuperLU (the bound of parity_cases.check_linear_solve)."""
    mo = pc.oracle_model(name)
    rng = np.random.default_rng(5)
    for periodic in (True, False):
        fd = corpus.synthetic_fields(name, N, seed=7, periodic=periodic, length=N * 5e-3)
        pars = corpus.synthetic_pars(name, N, periodic)
        n = N * len(mo._dep_vars)
        A = sps.identity(n, format="csc") - c * mo.J(mo.fields_template(**fd), pars)
        rhs = rng.standard_normal(n)
        xs = spla.spsolve(A, rhs)
        out = {}
        for narrow in (False, True):
            def run():
                solver = pc.bound_solver(pc.device_model(name, None), fd, pars, **opts)
                solver.eval(0, with_j=True)
                solver.factor(c)
                return solver.solve(rhs)[0].copy(), solver.describe()
            if narrow:
                with compilers.extra_flags(NARROW):
                    out[narrow] = run()
            else:
                out[narrow] = run()
        (xw, desc), (xn, desc0) = out[False], out[True]
        assert desc == desc0, (desc, desc0)
        e_wide, e_narrow = np.abs(xw - xs).max() / np.abs(xs).max(), np.abs(xn - xs).max() / np.abs(xs).max()
        same = np.array_equal(xw.view(np.uint64), xn.view(np.uint64))
        print("cr wide io solve %-8s N %d %s periodic %s: wide %.2e narrow %.2e (tol %.0e) bit-equal %s  [%s]"
              % (name, N, opts, periodic, e_wide, e_narrow, tol, same, desc))
        assert e_wide <= tol and e_narrow <= tol, (name, N, periodic, e_wide, e_narrow)
        assert same, (name, N, periodic, np.abs(xw - xn).max())
