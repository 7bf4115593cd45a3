"""Checks of the factored outermost block of the stored pivot rows, shared by the CPU emulation suite
(tests/test_u_outer.py) and the GPU suite (tests/test_gpu_u_outer.py).

A level-1 walk never touches a row's outermost block before that row is the pivot row, so the outermost
block of the normalised pivot row is Dinv times the block of A = I - c J as the value table gives it.
Where that is fewer values (codegen.outer_u_form: the film model, 4 stored + 1 loaded against 7) the
walks store the columns of Dinv that the block depends on and the back-substitutions rebuild it.  The
reference of every check is the same run with TRIFLOW_U_OUTER=0, where the generated header is the one
without the form and the kernels store and load the block itself:

  * the two runs are equal as values (numpy.array_equal: the terms the rebuilt product leaves out
    multiply exact zeros, which can only change the sign of a zero),
  * each lies within the bound of the oracle (oracle/numpy_path.py, SuperLU) that tests/block_mask_cases.py
    uses: film 2e-7, stiff 1e-9; a linear solve 1e-9 (tests/parity_cases.check_linear_solve).
"""
import numpy as np
import scipy.sparse as sps
import scipy.sparse.linalg as spla

from oracle import corpus, numpy_path as ora
from tests import block_mask_cases as bc
from tests import parity_cases as pc
from triflow_amd import Model, codegen
from triflow_amd.ensemble import Ensemble

FILM_TOL, STIFF_TOL, SOLVE_TOL = bc.FILM_TOL, bc.STIFF_TOL, 1e-9
assert FILM_TOL == 2e-7 and STIFF_TOL == 1e-9


# ------------------------------------------------------------------------------------------ lowering
def lowered(margs, **env):
    m = Model(*margs, compiler=lambda m: (None, None))
    return bc.with_env(env, lambda: codegen.lower_model(m))


def check_film_form():
    """S = {q, T}; one loaded plane feeds the block: d(q equation)/dh at offset -2, which the entry at +2
    is a power-of-two multiple of; (q, q) and (T, T) are node-independent and evaluated."""
    src, spec = lowered(corpus.model_args("M3_film"), TRIFLOW_U_OUTER="1", TRIFLOW_BLOCK_MASK="1")
    form = spec["u_outer"]
    assert form is not None and "#define TF_UOUT_FACT 1" in src
    h, q, T = 0, 1, 2
    want_nz = np.zeros((3, 3), dtype=bool)
    want_nz[q, h] = want_nz[q, q] = want_nz[T, T] = True
    for d, off in enumerate((2, -2)):
        assert form["rows"][d] == [False, True, True], form["rows"]
        assert np.array_equal(np.array(form["nz"][d]), want_nz), form["nz"]
        ks = [k for k in range(spec["nnz"]) if spec["pat_off"][k] == off]
        assert sorted((spec["pat_eq"][k], spec["pat_var"][k]) for k in ks) == [(q, h), (q, q), (T, T)]
        loaded = [k for k in ks if not spec["j_uniform"][k]]
        assert [(spec["pat_eq"][k], spec["pat_var"][k]) for k in loaded] == [(q, h)]
        plane = [spec["j_alias"][k] if spec["j_alias"][k] >= 0 else k for k in loaded]
        assert form["planes"][d] == plane and len(plane) == 1, (form["planes"], plane)
        # the count of the rule: 3 kept entries of Dinv[:, q], 1 of Dinv[:, T], 1 plane, against 7
        mask = np.array(spec["blk_nz"])
        assert int(mask[:, [q, T]].sum()) == 4 and int(mask.sum()) == 7
    # the switch: the header of the stored form
    src0, spec0 = lowered(corpus.model_args("M3_film"), TRIFLOW_U_OUTER="0", TRIFLOW_BLOCK_MASK="1")
    assert spec0["u_outer"] is None and "TF_UOUT" not in src0 and "tf_uout" not in src0
    assert src0 != src
    # the dense mask: 6 + 1 < 9, the rule still fires
    srcd, specd = lowered(corpus.model_args("M3_film"), TRIFLOW_U_OUTER="1", TRIFLOW_BLOCK_MASK="0")
    assert specd["u_outer"] is not None and specd["u_outer"]["rows"] == form["rows"]


#: models that keep the stored form: every equation reaches the outer offset (stiff, wave, tri3), rows are
#: exchanged (scalar), or the blocks are too wide for the registers (wide4)
STORED_MODELS = ["M5_stiff", "wave", "tri3", "M1_advdiff", "wide4"]


def check_stored_form_header(name):
    src1, spec1 = lowered(corpus.model_args(name), TRIFLOW_U_OUTER="1")
    src0, spec0 = lowered(corpus.model_args(name), TRIFLOW_U_OUTER="0")
    assert spec1["u_outer"] is None and spec0["u_outer"] is None
    assert src1 == src0 and "TF_UOUT" not in src1 and "tf_uout" not in src1, name


# ------------------------------------------------------------------------------------------ factored against stored
def device_state(backend, case, u_outer, margs=None, **env):
    name, x, fields, pars, dt = bc.member_inputs(case)

    def run():
        m = bc.make_model(margs or corpus.model_args(name), backend)
        ens = Ensemble(m, x, fields, pars, bool(pars["periodic"]), scheme=case["scheme"],
                       hook=bc.HOOKS[case.get("hook")][0], nstate=3, **case.get("opts", {}))
        assert (ens.solver.model.spec["u_outer"] is not None) == (u_outer == "1" and case.get("fires", True))
        for _ in range(case["steps"]):
            ens.step(dt)
        ens.sync()
        st = ens.state().copy()
        desc = ens.solver.describe()
        ens.close()
        return st, desc
    return bc.with_env(dict(env, TRIFLOW_U_OUTER=u_outer), run)


def check_factored_against_stored(backend, case, tol, **env):
    ref = bc.oracle_state(case)
    fact, desc = device_state(backend, case, "1", **env)
    stored, desc0 = device_state(backend, case, "0", **env)
    assert desc == desc0, (desc, desc0)
    assert fact.shape == ref.shape and np.isfinite(fact).all() and np.isfinite(stored).all(), case["id"]
    scale = np.abs(ref).max()
    e_fact, e_stored = np.abs(fact - ref).max() / scale, np.abs(stored - ref).max() / scale
    same = np.array_equal(fact, stored)
    print("u outer %-30s %s: factored %.2e stored %.2e (tol %.0e) equal %s  [%s]"
          % (case["id"], env or "", e_fact, e_stored, tol, same, desc))
    assert e_stored <= tol, (case["id"], env, "stored", e_stored)
    assert e_fact <= tol, (case["id"], env, "factored", e_fact)
    assert same, (case["id"], env, np.abs(fact - stored).max())


def _bc_name(periodic):
    return "per" if periodic else "clamp"


#: N = 203 (chunks of unequal length, a chunk count that is no multiple of 64) and 2100, periodic and clamped
#: (the fold at both ends), 1 and 3 members, ROS2 (the update inside the back-substitution) and RODASPR
#: (the plain solution)
FILM_GRID = [bc.film_case("uo_film_%d_%s_%dm_%s" % (N, _bc_name(periodic), nsys, sch), N, periodic, nsys, sch)
             for N in (203, 2100) for periodic in (True, False)
             for nsys, sch in ((1, "ROS2"), (3, "RODASPR"), (3, "ROS2"), (1, "RODASPR"))]
#: BDF2 with a Dirichlet hook
FILM_BDF2 = [bc.film_case("uo_film_%d_%s_%dm_BDF2_hook" % (N, _bc_name(periodic), nsys), N, periodic, nsys, "BDF2",
                          hook="film")
             for N, periodic, nsys in ((203, False, 1), (2100, False, 3), (203, True, 3), (2100, True, 1))]
#: the cases of the switches of the level-1 launches (3 members, ROS2: the twisted walks, the update inside
#: the back-substitution)
FILM_SWITCH = [c for c in FILM_GRID if c["nsys"] == 3 and c["scheme"] == "ROS2"]
#: N = 40 000 with 3 members: the split factorisation walk and the fused level-2 launches (GPU suite)
FILM_LARGE = bc.film_case("uo_film_40000_per_3m_ROS2", 40000, True, 3, "ROS2")
#: the stiff model keeps the stored form: the two runs are the same code
STIFF_CASE = dict(bc.stiff_case("uo_stiff_203", 203), fires=False)


# ------------------------------------------------------------------------------------------ one equation alone reaches +-2
#: u's equation reaches +-1, v's +-2: S = {v}.  2 kept entries of Dinv[:, v] + 1 plane (d/du_m2, which d/du_p2
#: is the negative of) against the 4 of the block
SYNTH_MODEL = (["-dxv", "u*dxxxu + k*dxxv"], ["u", "v"], ["k"], None)
SYNTH_C = 5e-3
#: the re-elimination form with both walks (default: only from TF_RESPIKE_MIN_NODES nodes on)
SYNTH_TWIST = dict(TRIFLOW_L1_RESPIKE="1", TRIFLOW_L1_TWIST="1")


def synth_inputs(N, periodic):
    x = np.arange(N) * 0.25
    L = N * 0.25
    u = 1.0 + 0.3 * np.cos(2 * np.pi * x / L) + 0.1 * np.sin(2 * np.pi * 5 * x / L)
    v = 0.5 * np.sin(2 * np.pi * 3 * x / L) - 0.2
    return dict(x=x, u=u, v=v), dict(k=0.3, periodic=periodic)


def check_synth_form():
    src, spec = lowered(SYNTH_MODEL, TRIFLOW_U_OUTER="1")
    form = spec["u_outer"]
    assert spec["mp"] == 2 and form is not None and "#define TF_UOUT_FACT 1" in src
    assert form["rows"] == [[False, True], [False, True]]
    assert all(len(p) == 1 for p in form["planes"])
    assert np.array(spec["blk_nz"]).all()


def check_synth_solve(backend, N, periodic, env=None, **opts):
    """One factorisation and one solve: factored == stored as values at every node -- with 4-node chunks every
    interior node is among the first or the last mp pivots of its chunk, where the outer column lies in a
    separator -- and both within SOLVE_TOL of SuperLU.  ``env``: switches of the level-1 launches; with
    SYNTH_TWIST the up walk stores the rows of its half, whose outer block is rebuilt from d/du_m2 itself
    where the down walk's takes the negative of it."""
    fd, pars = synth_inputs(N, periodic)
    mo = Model(*SYNTH_MODEL, compiler=ora.numpy_compiler)
    n = 2 * N
    A = sps.identity(n, format="csc") - SYNTH_C * mo.J(mo.fields_template(**fd), pars)
    rhs = np.random.default_rng(11).standard_normal(n)
    xs = spla.spsolve(A, rhs)
    out = {}
    for u_outer in ("1", "0"):
        def run():
            m = bc.make_model(SYNTH_MODEL, backend)
            solver = pc.bound_solver(m, fd, pars, refine=0, **opts)
            assert (solver.model.spec["u_outer"] is not None) == (u_outer == "1")
            solver.eval(0, with_j=True)
            solver.factor(SYNTH_C)
            return solver.solve(rhs)[0].copy(), solver.describe()
        out[u_outer] = bc.with_env(dict(env or {}, TRIFLOW_U_OUTER=u_outer), run)
    (xf, desc), (x0, desc0) = out["1"], out["0"]
    assert desc == desc0, (desc, desc0)
    e_fact, e_stored = np.abs(xf - xs).max() / np.abs(xs).max(), np.abs(x0 - xs).max() / np.abs(xs).max()
    same = np.array_equal(xf, x0)
    print("u outer synthetic N %d periodic %s %s %s: factored %.2e stored %.2e (tol %.0e) equal %s  [%s]"
          % (N, periodic, opts, env or "", e_fact, e_stored, SOLVE_TOL, same, desc))
    assert e_fact <= SOLVE_TOL and e_stored <= SOLVE_TOL, (e_fact, e_stored)
    assert same, np.abs(xf - x0).max()
