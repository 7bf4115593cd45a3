"""Checks of the two scalars that decide whether an adaptive run accepts a step, shared by the CPU emulation
suite (tests/test_reductions.py) and the GPU suite (tests/test_gpu_reductions.py):

* the step-doubling difference norm, ``tf_diff_norm`` (kernel ``tfk_diffnorm`` and the host fold of its
  partials), against an exact reference;
* the embedded Rosenbrock estimate, ``err_out`` of ``tf_step_row`` / ``tf_read_err`` (``tfk_vec_maxabs``);
* the state plane I/O both are measured through.

Bounds of the norms (derived, not measured).  ``d = A - B`` in float64 is the device's one rounding per element and
the reference starts from the same ``d``.  Maximum norm: no further rounding, so the result equals
``np.abs(d).max()`` bit for bit, NaN included.  Euclidean norm: every term ``d*d`` is non-negative, so a sum of n
terms in any order (fused or not) has a relative error of at most n u / (1 - n u), the square root halves it and adds
one rounding: ``|dev - exact| <= (N + 2) * 2**-53 * exact`` for every plan and for the emulation.  The entries of
one (variable, system) pair have comparable magnitudes, so a missed node, a doubled node or a padding element that
was counted moves the sum by ~1/N: nine orders of magnitude above the bound at N = 3001."""
import os
from fractions import Fraction
from functools import lru_cache, partial

import mpmath
import numpy as np

from oracle import corpus, numpy_path as ora
from triflow_amd import Model, device, schemes
from triflow_amd.compilers import hip_compiler
from triflow_amd.ensemble import Ensemble
from triflow_amd.tableaux import TABLEAUX

U53 = 2.0 ** -53
NORM_MODELS = ("M2_diff", "M3_film", "M5_stiff")             # 1, 3 and 5 variables
NORM_SIZES = (5, 9, 80, 203, 3001)                          # fewer nodes than workgroups; not ragged; ragged
RAGGED = (203, 3001)
#: (model, systems, nodes) of check_nonfinite_norms: one element per workgroup of the norm kernel; 11; 28
NONFINITE_CASES = [("M3_film", 2, 203), ("M3_film", 2, 3001), ("M5_stiff", 3, 3001)]


@lru_cache(maxsize=None)
def _model(name, backend):
    eqs, dep, pars, helps = corpus.model_args(name)
    compiler = hip_compiler if backend is None else partial(hip_compiler, backend=backend)
    return Model(eqs, dep, pars, helps, compiler=compiler)


def device_model(name, backend):
    return _model(name, backend)


def with_env(pairs, fn):
    """fn() with the environment variables of ``pairs`` set (solvers read their switches when created)."""
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


def ensemble(backend, name, N, nsys, periodic, scheme="ROS2", scale=None, **opts):
    """An Ensemble of ``nsys`` members of model ``name`` on synthetic fields (member e: the fields times scale[e])."""
    m = device_model(name, backend)
    fd = corpus.synthetic_fields(name, N, seed=7, periodic=periodic, length=N * 5e-2)
    pars = corpus.synthetic_pars(name, N, periodic)
    scale = (1.0 + 0.01 * np.arange(nsys)) if scale is None else np.asarray(scale, dtype=float)
    fields = {k: v[None, :] * scale[:, None] for k, v in fd.items() if k != "x"}
    opts.setdefault("nstate", 2)
    return Ensemble(m, fd["x"], fields, pars, periodic, scheme=scheme, **opts)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).tobytes()


# ====================================================================================== difference norms
@lru_cache(maxsize=None)
def norm_states(nvar, nsys, N, seed=0):
    """(A, B), [nvar][nsys][N]: signed entries of comparable magnitude inside one (variable, system) pair, and
    a scale of its own, 10**(v + nvar*e), for every pair -- a transposed out[nsys][nvar] is off by decades."""
    rng = np.random.default_rng([seed, nvar, nsys, N])
    scale = 10.0 ** (np.arange(nvar)[:, None] + nvar * np.arange(nsys)[None, :])
    A = scale[:, :, None] * rng.uniform(-1.0, 1.0, (nvar, nsys, N))
    B = scale[:, :, None] * rng.uniform(-1.0, 1.0, (nvar, nsys, N))
    A.setflags(write=False)
    B.setflags(write=False)
    return A, B


def exact_norm2(d):
    """sqrt of the exact sum of d*d (rational arithmetic, the root at 240 bits) of a finite 1-D array"""
    total = sum((Fraction(float(x)) ** 2 for x in d), Fraction(0))
    with mpmath.workprec(240):
        return mpmath.sqrt(mpmath.mpf(total.numerator) / mpmath.mpf(total.denominator))


def within_bound(value, exact, n):
    """|value - exact| <= (n + 2) u exact"""
    with mpmath.workprec(240):
        return abs(mpmath.mpf(float(value)) - exact) <= (n + 2) * mpmath.mpf(U53) * exact


def reference_norms(A, B):
    """(d, exact Euclidean norms [nsys][nvar] as mpmath numbers, maximum norms [nsys][nvar])"""
    d = np.asarray(A) - np.asarray(B)                                  # the one rounding the device makes too
    nvar, nsys, N = d.shape
    two = [[exact_norm2(d[v, e]) for v in range(nvar)] for e in range(nsys)]
    return d, two, np.abs(d).max(axis=2).T.copy()


@lru_cache(maxsize=None)
def reference_of_states(nvar, nsys, N):
    A, B = norm_states(nvar, nsys, N)
    d, two, inf = reference_norms(A, B)
    # np.linalg.norm on the same data stays inside the bound the device is held to
    for e in range(nsys):
        for v in range(nvar):
            assert within_bound(np.linalg.norm(d[v, e], 2), two[e][v], N), ("np.linalg.norm", nvar, nsys, N, e, v)
            assert np.linalg.norm(d[v, e], np.inf) == inf[e, v]
    return two, inf


def assert_norms(solver, A, B, what, ref=None):
    """Uploads A and B into slots 0 and 1 (None: what the slots hold) and holds both norms to the reference."""
    if A is not None:
        solver.set_state(0, A)
        solver.set_state(1, B)
    two, inf = ref if ref is not None else reference_norms(A, B)[1:]
    nsys, nvar = inf.shape
    got_inf = solver.diff_norms(0, 1, np.inf)
    got_two = solver.diff_norms(0, 1, 2)
    assert got_inf.shape == (nsys, nvar) and got_two.shape == (nsys, nvar), what
    assert np.array_equal(got_inf, inf, equal_nan=True) and not np.signbit(got_inf).any(), (what, "max norm", got_inf, inf)
    for e in range(nsys):
        for v in range(nvar):
            assert within_bound(got_two[e, v], two[e][v], solver.N), \
                (what, "2-norm of variable %d, system %d" % (v, e), got_two[e, v], float(two[e][v]),
                 "relative error %.3e, bound %.3e" % (abs(got_two[e, v] - float(two[e][v])) / float(two[e][v]),
                                                      (solver.N + 2) * U53))
    return got_two, got_inf


def norm_solver(backend, name, nsys, N, periodic, **opts):
    """A solver with two state slots or more: the members of an Ensemble, or the one system of bound_solver.
    release() closes either."""
    if nsys > 1:
        return ensemble(backend, name, N, nsys, periodic, **opts).solver
    from tests.parity_cases import bound_solver
    m = device_model(name, backend)
    fd = corpus.synthetic_fields(name, N, seed=7, periodic=periodic, length=N * 5e-2)
    return bound_solver(m, fd, corpus.synthetic_pars(name, N, periodic), nstate=2, **opts)


def release(backend, name, solver):
    """Closes a solver of norm_solver; one of bound_solver also leaves the compiled model's per-shape cache, so
    that no later caller is handed a closed solver."""
    cache = device_model(name, backend)._device._solvers
    for key in [k for k, v in cache.items() if v is solver]:
        del cache[key]
    solver.close()


def check_diff_norms(backend, name, nsys):
    """tf_diff_norm of random states against the exact reference: every size, periodic and clamped, and an
    explicit 7-node plan at N = 203; at the ragged sizes the default plan's padding row is really read."""
    nvar = len(corpus.field_names(name)[0])
    for N in NORM_SIZES:
        A, B = norm_states(nvar, nsys, N)
        ref = reference_of_states(nvar, nsys, N)
        for periodic in (True, False):
            for opts in ((dict(), dict(m1=7)) if N == 203 else (dict(),)):
                s = norm_solver(backend, name, nsys, N, periodic, **opts)
                P = s.describe()["chunks"][0]
                if opts:                                  # (29 chunks of 7 nodes: another plan, not ragged)
                    assert N == 7 * P, (name, N, opts, s.describe())
                elif N in RAGGED:
                    assert N % P != 0, (name, N, opts, s.describe())
                assert_norms(s, A, B, (name, nsys, N, periodic, opts, s.describe()["chunks"]), ref)
                release(backend, name, s)


def check_padding_after_steps(backend, N, periodic=True):
    """Three ROS2 steps and two Theta steps of two film members leave states in slots 0 and 1; the device norms of
    their difference meet the bounds against the two downloaded states.  Allocation zero-fills the planes and the
    vector kernels and the norm run over them whole: this fails if any kernel of a step leaves something in the
    padding of a state plane."""
    ens = ensemble(backend, "M3_film", N, 2, periodic, nstate=2)
    s, tab, dt = ens.solver, TABLEAUX["ROS2"], 1e-3
    assert N % s.describe()["chunks"][0] != 0, s.describe()
    for src, dst in ((0, 1), (1, 0), (0, 1)):
        s.step_row(src, dst, dt, tab.alpha, tab.gamma, tab.b, None, hook_after=True, want_err=False)
    s.step_theta(1, 0, dt, 1.0)
    s.step_theta(0, 1, dt, 0.5)
    A, B = s.get_state(0), s.get_state(1)
    assert np.isfinite(A).all() and np.isfinite(B).all() and not np.array_equal(A, B)
    assert_norms(s, None, None, ("after steps", N, periodic), reference_norms(A, B)[1:])
    ens.close()


def last_row_node(solver):
    """A node stored in the last row of the planes (the row that is padding for the shorter chunks): the last
    node of chunk 0, which is one node longer than the base length"""
    P = solver.describe()["chunks"][0]
    assert solver.N % P != 0
    return solver.N // P


def lane_nodes(solver):
    """Nodes that tfk_diffnorm reads in lanes 1, 2, per/2 and per - 1 of a workgroup's first wavefront, where a NaN
    has to cross the shuffle fold to reach lane 0.  diff_norm (tf_rt_steps.cpp) launches nb workgroups per
    (variable, system) pair over the M * P elements of a plane, ``per`` consecutive ones each, thread t element
    blk * per + t: row q / P of chunk q % P.  (At N = 203 per is 1: only lane 0 ever holds a value.)"""
    nvs = solver.nvar * solver.nsys
    nb = min(1024, max(64, 2048 // nvs))
    P = solver.describe()["chunks"][0]
    mbase, rem = divmod(solver.N, P)
    per = -(-(mbase + (rem > 0)) * P // nb)
    assert 4 <= per <= 64, (per, nb, P)
    nodes = []
    for k, t in enumerate((1, 2, per // 2, per - 1)):
        i, c = divmod((3 + 11 * k) * per + t, P)
        assert i < mbase, (i, mbase)
        nodes.append(c * mbase + min(c, rem) + i)
    return nodes


def special_cases(N, nan_nodes, both_node=None):
    """(id, [(array, variable, system, node, value)], {(system, variable): (2-norm, max norm)} expected where they
    differ from the unmodified run).  One entry per run; inf - inf at ``both_node``."""
    nan, inf = np.nan, np.inf
    both_node = N - 1 if both_node is None else both_node
    last_row = nan_nodes[2]
    cases = []
    for k, node in enumerate(nan_nodes):
        v, e = k % 3, k % 2
        cases.append(("nan_node_%d" % node, [("A", v, e, node, nan)], {(e, v): (nan, nan)}))
    cases.append(("inf_in_A", [("A", 1, 1, 17, inf)], {(1, 1): (inf, inf)}))
    cases.append(("neg_inf_in_A", [("A", 2, 0, last_row, -inf)], {(0, 2): (inf, inf)}))
    cases.append(("inf_in_both", [("A", 0, 1, both_node, inf), ("B", 0, 1, both_node, inf)], {(1, 0): (nan, nan)}))
    # d = 1e200: its square overflows, as in np.linalg.norm
    cases.append(("huge", [("A", 1, 0, 5, 1e200), ("B", 1, 0, 5, 0.0)], {(0, 1): (inf, 1e200)}))
    return cases


def check_nonfinite_norms(backend, name="M3_film", nsys=2, N=203):
    """Non-finite and signed values, both norms: a NaN anywhere in a (variable, system) pair makes that pair's norms
    NaN -- the first node, the last, one in the last plane row, one in the middle -- and leaves every other pair's
    bits alone; +-inf gives inf; inf - inf gives NaN; a difference whose square overflows gives inf / itself; equal
    states with mixed signed zeros give +0.0; subnormal differences give what NumPy gives.

    What each size can see.  At N = 203 every workgroup of tfk_diffnorm reads one element, in lane 0: the cases hold
    the per-thread maximum and the host fold of the partials, on both tiers.  At N = 3001 a workgroup reads 11
    (3 x 2 pairs) or 28 (5 x 3) elements, and the NaN / inf - inf nodes are chosen in lanes other than 0
    (lane_nodes): on the GPU they also hold the wavefront shuffle fold, which the emulation does not have.  The fold
    over a workgroup's four wavefronts is held by no case: a second wavefront reads something only with more than
    64 elements per workgroup, above 4096 nodes at the fewest workgroups there are (64); at these sizes its
    operands part[1..3] are zeros.  That fold has the same expression as the shuffle fold, by reading."""
    nvar = len(corpus.field_names(name)[0])
    s = norm_solver(backend, name, nsys, N, True)
    A0, B0 = norm_states(nvar, nsys, N)
    base_two, base_inf = assert_norms(s, A0, B0, "base", reference_of_states(nvar, nsys, N))
    if N == 203:
        cases = special_cases(N, (0, N - 1, last_row_node(s), N // 2))
    else:
        lanes = lane_nodes(s)
        cases = special_cases(N, (0, N - 1, last_row_node(s)) + tuple(lanes), both_node=lanes[1])
    for cid, edits, expect in cases:
        A, B = A0.copy(), B0.copy()
        for which, v, e, node, value in edits:
            (A if which == "A" else B)[v, e, node] = value
        s.set_state(0, A)
        s.set_state(1, B)
        want_two, want_inf = base_two.copy(), base_inf.copy()
        for (e, v), (w2, wi) in expect.items():
            want_two[e, v], want_inf[e, v] = w2, wi
        got_inf, got_two = s.diff_norms(0, 1, np.inf), s.diff_norms(0, 1, 2)
        # NaN where expected (whatever its payload), every other entry bit for bit
        for got, want, ord_ in ((got_inf, want_inf, "inf"), (got_two, want_two, 2)):
            assert np.array_equal(np.isnan(got), np.isnan(want)), (cid, ord_, got, want)
            keep = ~np.isnan(want)
            assert bits(got[keep]) == bits(want[keep]), (cid, ord_, got, want)
        with np.errstate(all="ignore"):                       # and NumPy agrees on the edited pair
            d = A - B
            for (e, v) in expect:
                assert np.array_equal(np.linalg.norm(d[v, e], np.inf), got_inf[e, v], equal_nan=True), cid
                assert np.array_equal(np.linalg.norm(d[v, e], 2), got_two[e, v], equal_nan=True), cid
    # A == B with mixed signed zeros: +0.0, both norms
    A = A0.copy()
    A[:, :, ::3] = 0.0
    A[:, :, 1::7] = -0.0
    B = A.copy()
    B[:, :, ::6] = -0.0                  # (+0 against -0, -0 against -0, -0 against +0, +0 against +0)
    B[:, :, 1::14] = 0.0
    assert np.array_equal(A, B) and bits(A) != bits(B)
    s.set_state(0, A)
    s.set_state(1, B)
    for ord_ in (np.inf, 2):
        assert bits(s.diff_norms(0, 1, ord_)) == bits(np.zeros((nsys, nvar))), ord_
    # subnormal differences: the maximum exactly; their squares underflow, in NumPy as on the device
    rng = np.random.default_rng(3)
    A = rng.integers(1, 2 ** 20, (nvar, nsys, N)) * 5e-324
    B = rng.integers(1, 2 ** 20, (nvar, nsys, N)) * 5e-324
    d = A - B
    assert (np.abs(d) < np.finfo(float).tiny).all() and (d != 0).any()
    s.set_state(0, A)
    s.set_state(1, B)
    assert bits(s.diff_norms(0, 1, np.inf)) == bits(np.abs(d).max(axis=2).T)
    assert bits(s.diff_norms(0, 1, 2)) == bits(np.linalg.norm(d, 2, axis=2).T)
    release(backend, name, s)


def check_scheme_difference_norms(backend):
    """schemes._difference_norms on device-backed containers (the reduction kernel) against the host branch of the
    same function on the same states, the special values included: the maximum norm bit for bit, NaN for NaN; the
    Euclidean norm equal where it is not finite, and both branches inside the bound of the exact value elsewhere."""
    name, N = "M3_film", 203
    m = device_model(name, backend)
    dep = list(m._dep_vars)
    x = np.linspace(0, 10, N, endpoint=False)
    pars = corpus.synthetic_pars(name, N, True)
    A0, B0 = norm_states(3, 2, N)

    # Device-backed containers of given states.  The public way to one is a step of a scheme, which would change the
    # state (no scheme takes a step of length 0 that leaves the bits alone), so the states are placed the way
    # schemes._device_step places an uploaded input: the model's cached Stepper, acquire (upload into a free
    # slot), wrap (the container a step returns).
    def containers(U):
        host = m.fields_template(x=x, **{k: U[v] for v, k in enumerate(dep)})
        stepper = device.stepper_for(m, host, pars)
        stepper.bind(host, pars)
        return host, stepper.wrap(host, stepper.acquire(host))

    _, first = containers(A0[:, 0, :])
    P = first._device_backing().stepper.solver.describe()["chunks"][0]
    assert N % P != 0
    for cid, edits, _ in [("plain", [], None)] + special_cases(N, (0, N - 1, N // P, N // 2)):
        A, B = A0[:, 0, :].copy(), B0[:, 0, :].copy()
        for which, v, e, node, value in edits:
            (A if which == "A" else B)[v, node] = value                 # (the one system of a scheme's solver)
        ha, da = containers(A)
        hb, db = containers(B)
        assert da._device_backing() is not None and db._device_backing() is not None
        assert da._device_backing().stepper is db._device_backing().stepper
        with np.errstate(all="ignore"):
            for ord_ in (np.inf, 2):
                dev = np.array(schemes._difference_norms(da, db, ord_))
                host = np.array(schemes._difference_norms(ha, hb, ord_))
                assert da._device_backing() is not None and db._device_backing() is not None      # nothing came down
                if ord_ == np.inf:
                    assert np.array_equal(dev, host, equal_nan=True), (cid, dev, host)
                    continue
                finite = np.isfinite(host)
                assert np.array_equal(dev[~finite], host[~finite], equal_nan=True), (cid, dev, host)
                for v in np.nonzero(finite)[0]:
                    exact = exact_norm2(A[v] - B[v])
                    assert within_bound(dev[v], exact, N) and within_bound(host[v], exact, N), (cid, v, dev, host)


# ====================================================================================== embedded estimate
EST_CASES = [("film_per", 3, True), ("film_clamp", 3, False), ("diff_per", 2, True)]
EST_TABLEAUX = ("ROS3PRw", "RODASPR")
N_EST = 203
#: Relative difference between the library's estimate and the oracle's (SuperLU): bounded by the two solvers'
#: cond * eps, so it is measured -- profiles/r10_reductions.txt: at most MEASURED_EST_DIFF on the MI355X and on the
#: emulation -- and asserted at 100 x the larger measured value, not below 100 eps.
MEASURED_EST_DIFF = 3.52e-15
EST_TOL = max(100 * MEASURED_EST_DIFF, 100 * np.finfo(float).eps)


def est_inputs(cfg, periodic):
    name, fd, pars, dt, _ = corpus.config_inputs(cfg, N_EST)
    return name, fd, dict(pars, periodic=periodic), dt


def est_ensemble(backend, cfg, periodic, scale=(1.0,), **opts):
    """Members of config ``cfg`` at N_EST nodes, member e: the initial fields times scale[e]"""
    name, fd, pars, dt = est_inputs(cfg, periodic)
    m = device_model(name, backend)
    scale = np.asarray(scale, dtype=float)
    fields = {k: v[None, :] * scale[:, None] for k, v in fd.items() if k != "x"}
    opts.setdefault("nstate", 2)
    return Ensemble(m, fd["x"], fields, pars, periodic, scheme="ROS2", **opts), dt


def row_step(s, tab, dt, src=0, dst=1, err_slot=None):
    if err_slot is None:
        return s.step_row(src, dst, dt, tab.alpha, tab.gamma, tab.b, b_pred=tab.b_pred)
    s.step_row_queued(src, dst, dt, tab.alpha, tab.gamma, tab.b, tab.b_pred, err_slot=err_slot)
    return s.read_err(err_slot)


def estimate_against_oracle(backend):
    """[(case, tableau, library, oracle, relative difference)]: err_out of tf_step_row against ||U - U_pred||_inf of
    the oracle's _fixed_step (SuperLU) on the same inputs"""
    rows = []
    for cid, cfg, periodic in EST_CASES:
        name, fd, pars, dt = est_inputs(cfg, periodic)
        mo = Model(*corpus.model_args(name), compiler=ora.numpy_compiler)
        for tname in EST_TABLEAUX:
            _, _, want = getattr(ora, tname)(mo)._fixed_step(0.0, mo.fields_template(**fd), dt, pars)
            ens, _ = est_ensemble(backend, cfg, periodic)
            got = row_step(ens.solver, TABLEAUX[tname], dt)
            ens.close()
            rows.append((cid, tname, float(got), float(want), abs(float(got) - float(want)) / float(want)))
    return rows


def check_estimate_against_oracle(backend):
    rows = estimate_against_oracle(backend)
    for cid, tname, got, want, rel in rows:
        print("embedded estimate %-10s %-8s library %.17e oracle %.17e relative difference %.2e" % (cid, tname, got, want, rel))
    for cid, tname, got, want, rel in rows:
        assert want > 0 and np.isfinite(got) and rel <= EST_TOL, (cid, tname, got, want, rel, EST_TOL)


def check_estimate_is_the_maximum_over_members(backend):
    """err_out is one scalar over all systems: with two members of different initial states it is the maximum of
    the two single-member runs' estimates bit for bit (the same level plan: m1 fixed), whichever member holds
    it; and the members' new states are those of the single runs."""
    for cid, cfg, periodic in EST_CASES:
        for tname in EST_TABLEAUX:
            tab = TABLEAUX[tname]
            single = {}
            for sc in (1.0, 1.3):
                ens, dt = est_ensemble(backend, cfg, periodic, (sc,), m1=8)
                single[sc] = (row_step(ens.solver, tab, dt), ens.solver.get_state(1))
                ens.close()
            assert single[1.0][0] != single[1.3][0] and all(np.isfinite(v[0]) and v[0] > 0 for v in single.values())
            for scales in ((1.0, 1.3), (1.3, 1.0)):
                ens, dt = est_ensemble(backend, cfg, periodic, scales, m1=8)
                err = row_step(ens.solver, tab, dt)
                new = ens.solver.get_state(1)
                ens.close()
                assert bits(err) == bits(max(single[sc][0] for sc in scales)), (cid, tname, scales, err, single)
                for e, sc in enumerate(scales):
                    assert np.array_equal(new[:, e, :], single[sc][1][:, 0, :]), (cid, tname, scales, e)


def check_estimate_queued_equals_blocking(backend):
    """tf_step_row_queued + tf_read_err return the bits of tf_step_row's err_out and leave its state, in reduction
    slot 1, 2 and 3; three steps queued back to back keep their estimates apart, read in any order."""
    for cid, cfg, periodic in EST_CASES:
        for tname in EST_TABLEAUX:
            tab = TABLEAUX[tname]
            ens, dt = est_ensemble(backend, cfg, periodic, (1.0, 1.1))
            s = ens.solver
            U0 = s.get_state(0)
            dts = {1: dt, 2: 0.5 * dt, 3: 2.0 * dt}
            blocking = {}
            for slot, h in dts.items():
                s.set_state(0, U0)
                blocking[slot] = (row_step(s, tab, h), s.get_state(1))
            assert len({bits(v[0]) for v in blocking.values()}) == 3
            for slot, h in dts.items():
                s.set_state(0, U0)
                err = row_step(s, tab, h, err_slot=slot)
                assert bits(err) == bits(blocking[slot][0]), (cid, tname, slot, err, blocking[slot][0])
                assert np.array_equal(s.get_state(1), blocking[slot][1]), (cid, tname, slot)
            s.set_state(0, U0)
            for slot, h in dts.items():
                s.step_row_queued(0, 1, h, tab.alpha, tab.gamma, tab.b, tab.b_pred, err_slot=slot)
            for slot in (3, 1, 2):
                assert bits(s.read_err(slot)) == bits(blocking[slot][0]), (cid, tname, "back to back", slot)
            ens.close()


def check_estimate_fused_update_switch(backend):
    """TRIFLOW_FUSE_UPDATE=0 and 1 give the same estimate bits and the same new state.  An adaptive step never has
    its update inside the back-substitution (tf_rt_steps.cpp, step_row): with either value of the switch the estimate
    comes from one launch of tfk_vec_maxabs per step, which also forms the new state (TF_VEC_SUM_ERR), and tfk_vec is
    not launched -- the timing report shows it.  Returns the reports of the two solvers, and those of a fixed ROS2
    step on them (the step the switch is for)."""
    out = []
    for cid, cfg, periodic in EST_CASES:
        for tname in EST_TABLEAUX + ("ROS2",):
            tab = TABLEAUX[tname]
            # (two stages with an error estimate: the shape of step the fused update exists for)
            b_pred = tab.b_pred if tab.b_pred is not None else [0.25, -0.25]
            runs = []
            for fuse in ("1", "0"):
                def run():
                    ens, dt = est_ensemble(backend, cfg, periodic, (1.0, 1.1), m1=13, refine=0)
                    s = ens.solver
                    s.timing(True)
                    errs = []
                    for src, dst in ((0, 1), (1, 0), (0, 1)):
                        errs.append(s.step_row(src, dst, dt, tab.alpha, tab.gamma, tab.b, b_pred=b_pred))
                    state = s.get_state(1)
                    rep = s.timing_report()
                    s.timing_reset()
                    r2 = TABLEAUX["ROS2"]
                    s.step_row(1, 0, dt, r2.alpha, r2.gamma, r2.b, None, hook_after=True, want_err=False)
                    s.sync()
                    fixed = s.timing_report()
                    ens.close()
                    return errs, state, rep, fixed
                runs.append(with_env({"TRIFLOW_FUSE_UPDATE": fuse, "TRIFLOW_L1_RESPIKE": "1"}, run))
            (e1, s1, rep1, fix1), (e0, s0, rep0, fix0) = runs
            assert all(np.isfinite(e) and e > 0 for e in e1), (cid, tname, e1)
            assert bits(e1) == bits(e0), (cid, tname, e1, e0)
            assert np.array_equal(s1, s0), (cid, tname)
            for rep in (rep1, rep0):
                assert rep["tfk_vec_maxabs"][1] == 3 and "tfk_vec" not in rep, (cid, tname, sorted(rep))
            out.append((cid, tname, fix1, fix0))
    return out


#: What the library does with a NaN in one member's state (observed on the MI355X and on the emulation,
#: profiles/r10_reductions.txt; stated at tf_step_row in include/triflow_hip.h).  Blocking form (key None):
#: RuntimeError, the factorisation reports a non-finite pivot block.  Queued form (key: the reduction slot):
#: tf_read_err returns NaN -- it looks at the failure flag as it stood behind the step, and that one is not
#: raised -- and the next synchronising call, the download of the state, raises.
NAN_MEMBER_BEHAVIOUR = {None: "raises: pivot", 2: "nan, then the download raises"}


def check_estimate_nan_member(backend):
    """A NaN in one node of member 1's initial state: the step must return a NaN estimate or raise RuntimeError,
    never return a finite estimate.  Returns what the library did, {(case, tableau, form): behaviour}; where the
    call and the download both return, member 0's new state equals its NaN-free run bit for bit."""
    seen = {}
    for cid, cfg, periodic in EST_CASES:
        for tname in EST_TABLEAUX:
            tab = TABLEAUX[tname]
            ens, dt = est_ensemble(backend, cfg, periodic, (1.0, 1.1), m1=8)
            clean_err = row_step(ens.solver, tab, dt)
            clean = ens.solver.get_state(1)
            ens.close()
            assert np.isfinite(clean_err)
            for queued in (None, 2):
                ens, dt = est_ensemble(backend, cfg, periodic, (1.0, 1.1), m1=8)
                s = ens.solver
                U0 = s.get_state(0)
                U0[-1, 1, N_EST // 2] = np.nan
                s.set_state(0, U0)
                try:
                    err = row_step(s, tab, dt, err_slot=queued)
                except RuntimeError as ex:
                    kind = [k for k in ("pivot", "accuracy") if k in str(ex)]
                    assert kind, ex
                    seen[cid, tname, queued] = "raises: " + kind[0]
                else:
                    assert np.isnan(err), (cid, tname, queued, err)
                    try:
                        new = s.get_state(1)
                    except RuntimeError:
                        seen[cid, tname, queued] = "nan, then the download raises"
                    else:
                        seen[cid, tname, queued] = "nan, member 0 intact"
                        assert np.array_equal(new[:, 0, :], clean[:, 0, :]), (cid, tname, queued)
                        assert np.isnan(new[:, 1, :]).any()
                ens.close()
    return seen


# ====================================================================================== state plane I/O
def io_payload(nvar, nsys, N, seed=5):
    """[nvar][nsys][N] of distinct values with a NaN of non-default mantissa, -0.0, +-inf and subnormals among
    them, also at the first and the last node and in the last plane row"""
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((nvar, nsys, N))
    flat = a.reshape(-1).view(np.uint64)
    special = np.array([0x7ff8dead0000beef, 0xfff8000000000123, 0x8000000000000000, 0x0000000000000001,
                        0x800fffffffffffff, 0x7ff0000000000000, 0xfff0000000000000], dtype=np.uint64)
    where = rng.choice(flat.size, 4 * special.size, replace=False)
    flat[where] = np.tile(special, 4)
    flat[0], flat[N - 1], flat[flat.size - 1] = special[0], special[2], special[3]
    return a


def check_state_io(backend):
    """Round trips of the state planes at a ragged size (N = 203, nvar 3, nsys 2) return the input's bytes: SoA, AoS,
    the variable windows; the AoS download of an SoA upload is the [node * nvar + var] interleave; poke / peek with
    node 0, -1 and N - 1 hit the nodes NumPy indexing hits, in every system."""
    N, nvar, nsys = 203, 3, 2
    s = norm_solver(backend, "M3_film", nsys, N, False, nstate=3)
    assert N % s.describe()["chunks"][0] != 0
    a = io_payload(nvar, nsys, N)
    s.set_state(0, a)
    assert bits(s.get_state(0)) == bits(a)
    # [nsys][N * nvar], element node * nvar + var
    flat = np.ascontiguousarray(a.transpose(1, 2, 0)).reshape(nsys, N * nvar)
    assert bits(s.get_state_flat(0)) == bits(flat)
    b = io_payload(nvar, nsys, N, seed=6)
    flat_b = np.ascontiguousarray(b.transpose(1, 2, 0)).reshape(nsys, N * nvar)
    s.set_state_flat(1, flat_b)
    assert bits(s.get_state_flat(1)) == bits(flat_b) and bits(s.get_state(1)) == bits(b)
    assert bits(s.get_state(0)) == bits(a)                       # (the other slot is untouched)
    # windows: variables 1 and 2 replaced, variable 0 kept; and read back as a window
    s.set_state(0, b[1:3], first=1)
    want = np.concatenate([a[:1], b[1:3]])
    assert bits(s.get_state(0)) == bits(want)
    assert bits(s.get_state(0, first=1, nvars=2)) == bits(b[1:3])
    assert bits(s.get_state(0, first=2, nvars=1)) == bits(b[2:3])
    s.copy_state(0, 2)
    assert bits(s.get_state(2)) == bits(want)
    # point writes and reads
    want = want.copy()
    for k, node in enumerate((0, -1, N - 1, 1, N // 2)):
        v = k % nvar
        value = -0.0 if node == -1 else 1000.0 + k
        s.poke(0, [(v, node, value)])
        want[v, :, node] = value
        got = s.get_state(0)
        assert bits(got) == bits(want), (node, np.argwhere(got != want))
        for vv in range(nvar):
            assert bits(s.peek(0, vv, node)) == bits(want[vv, :, node]), (vv, node)
    s.close()
