"""What the CPU and the GPU suite of the exact Heaviside / DiracDelta / Piecewise mode share
(tests/test_heaviside.py on the emulation back end, tests/test_gpu_heaviside.py on the MI355X): the models,
states that sit on every kink, and the NumPy reference -- ``lambdify`` of the model's own SymPy arrays with
``Heaviside = numpy.heaviside`` and ``DiracDelta = 0`` on the ghost-padded views of the oracle
(DESIGN.md section 20)."""
from functools import partial

import numpy as np
from sympy import lambdify

from oracle import numpy_path as ora
from triflow_amd import Model, probes, schemes
from triflow_amd.compilers import hip_compiler

#: the reference's meaning of the two names NumPy's printer leaves alone (the test's own dictionary, not
#: the package's)
EXACT = [{"Heaviside": np.heaviside, "DiracDelta": lambda a, *_: np.zeros_like(a)}, "numpy"]

MODELS = {
    "burgers_up": ("k*dxxU - upwind(U, U, 2)", "U", ["k"]),
    "step_x": ("k*dxxU - Heaviside(x - 0.5, 0)*c*dxU", "U", ["k", "c"]),
    "gate": (["k*dxxU + Heaviside(V - 1)*U", "k*dxxV - U*V"], ["U", "V"], ["k"]),
    "pw": ("Piecewise((k*dxxU, (U > 0) & (U <= c)), (-c*dxU, True))", "U", ["k", "c"]),
    "pw_nan": ("Piecewise((k*dxxU, U > 0), (-c*dxU, U < -0.5))", "U", ["k", "c"]),
}
MODEL_GRIDS = [50, 1031]            # less than one sweep workgroup; ragged, several workgroups of 512 nodes
OBSERVER_GRIDS = [50, 1031, 2053]   # ... and ragged across an observer workgroup of 2048 nodes
C0 = 0.75                           # the threshold of pw, inside the range of U

_CACHE = {}


def model(name, mode="exact", backend=None, oracle=False):
    """A model of the table: on the HIP path (``backend=None``), on a test back end, or uncompiled."""
    key = (name, mode, id(backend), oracle)
    if key not in _CACHE:
        kw = {} if mode is None else dict(heaviside=mode)
        if oracle:
            _CACHE[key] = Model(*MODELS[name], hold_compilation=True, **kw)
        else:
            compiler = hip_compiler if backend is None else partial(hip_compiler, backend=backend)
            _CACHE[key] = Model(*MODELS[name], compiler=compiler, **kw)
    return _CACHE[key]


def _up(v):
    return np.nextafter(v, np.inf)


def _down(v):
    return np.nextafter(v, -np.inf)


def state(name, N, periodic, per_node):
    """(fields dict with x, parameter dict).  Smooth fields with noise; from node 3 on, three nodes apart
    (their stencils hold finite neighbours only), and again in the last 50 nodes of a longer grid: +0.0,
    -0.0, the smallest numbers either side of zero, the thresholds c, -0.5 and 1 exactly (ties of the
    comparisons, a zero argument of Heaviside(V - 1)) and one ulp either side; further on one NaN, +inf
    and -inf."""
    _, dep, pars = MODELS[name]
    rng = np.random.default_rng(N + 2 * periodic + per_node)
    x = np.linspace(0.0, 1.0, N, endpoint=not periodic)
    c = C0 + 0.1 * np.cos(2 * np.pi * x * 3) if per_node else np.float64(C0)
    k = 1e-3 * (1 + 0.5 * np.sin(2 * np.pi * x)) if per_node else 1e-3
    U = np.sin(2 * np.pi * x) + 0.2 + 0.05 * rng.standard_normal(N)
    V = 1.0 + 0.5 * np.cos(2 * np.pi * x) + 0.05 * rng.standard_normal(N)
    for base in ([0] if N < 100 else [0, N - 50]):
        cn = (lambda i: c[base + i]) if per_node else (lambda i: c)
        for i, v in ((3, 0.0), (6, -0.0), (9, _up(0.0)), (12, _down(0.0)), (15, cn(15)), (18, _up(cn(18))),
                     (21, _down(cn(21))), (24, -0.5), (27, _up(-0.5)), (30, _down(-0.5)),
                     (35, np.nan), (40, np.inf), (45, -np.inf)):
            U[base + i] = v
        for i, v in ((3, 1.0), (6, _up(1.0)), (9, _down(1.0)), (35, np.inf), (40, -np.inf), (45, np.nan)):
            V[base + i] = v
    fields = dict(x=x, U=U)
    if "V" in dep:
        fields["V"] = V
    p = dict(k=k, periodic=periodic)
    if "c" in pars:
        p["c"] = c
    return fields, p


def same_bits(a, b):
    """Equal bit for bit, but that every NaN equals every NaN: the values, and the signs of the zeros."""
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    if a.shape != b.shape:
        return False
    nan = np.isnan(a)
    return bool(np.array_equal(nan, np.isnan(b)) and np.array_equal(a[~nan], b[~nan])
                and np.array_equal(np.signbit(a[~nan]), np.signbit(b[~nan])))


def _inputs(m, fields, pars):
    return [np.asarray(fields["x"])] + [np.asarray(fields[k]) for k in m._dep_vars] + \
        [pars[k] for k in m._pars] + [pars["periodic"]]


def numpy_rows(m, exprs, fields, pars, modules=None):
    """[rows][N]: the lambdified expressions on the ghost-padded views of the oracle."""
    func = lambdify(m._symbolic_args, list(exprs), modules=modules or EXACT)
    env, N, _, _ = ora.stencil_views(m, *_inputs(m, fields, pars))
    with np.errstate(all="ignore"):
        vals = func(*[env[k] for k in m._args])
    return np.array([np.broadcast_to(np.asarray(v, dtype=float), (N,)) for v in vals])


def numpy_FJ(m, fields, pars):
    return (numpy_rows(m, m.F_array.tolist(), fields, pars),
            numpy_rows(m, m._J_sparse_array.tolist(), fields, pars))


def numpy_nodes(m, exprs, fields, pars):
    """The per-node values of observer expressions (strings of the model's language)."""
    return numpy_rows(m, [probes.discretise(m, e) for e in exprs], fields, pars)


def device_FJ(m, fields, pars):
    """F [nvar][N] and the raw Jacobian value table [nnz][N] from the kernels."""
    cm = m._device
    values = [pars[k] for k in cm.pars]
    N = fields["x"].size
    solver = cm.solver(N, pars["periodic"], 1, cm.parvec_mask_of(values))
    cm.bind_inputs(solver, fields["x"], values, None)
    solver.set_state(0, np.array([fields[k] for k in m._dep_vars]))
    solver.eval(0, with_j=True)
    F = np.array(solver.get_F()[0]).reshape(N, m._nvar).T
    J = np.array(solver.get_J()[0]).reshape(N, -1).T
    return F, J


def check_FJ(name, backend, N, periodic, per_node):
    m = model(name, "exact", backend)
    fields, pars = state(name, N, periodic, per_node)
    F, J = device_FJ(m, fields, pars)
    Fn, Jn = numpy_FJ(m, fields, pars)
    tag = (name, N, periodic, per_node)
    # (the special values of the state do reach the result)
    assert np.isnan(Fn).any() and (np.isinf(Fn).any() or np.isinf(Jn).any()), tag
    assert same_bits(F, Fn), (tag, np.argwhere(~((F == Fn) | (np.isnan(F) & np.isnan(Fn))))[:8])
    assert same_bits(J, Jn), (tag, np.argwhere(~((J == Jn) | (np.isnan(J) & np.isnan(Jn))))[:8])
    if name == "pw_nan":
        U = fields["U"]
        none = ~(U > 0) & ~(U < -0.5)
        assert none.sum() >= 5 and np.isnan(F[0][none]).all() and np.isnan(J[:, none]).all(), tag
        assert not np.isnan(F[0][:3]).any()


# ---------------------------------------------------------------------------------- the order of the step
ORDER_N, ORDER_K = 64, 1e-3
ORDER_DTS = (2e-3, 1e-3, 5e-4)


def order_state():
    x = np.linspace(0.0, 1.0, ORDER_N, endpoint=False)
    return dict(x=x, U=np.sin(2 * np.pi * x) + 0.2), dict(k=ORDER_K, periodic=True)


def dense_FJ(m):
    """(F(U), J(U)) of the exact semantics in dense NumPy, for the Newton iteration of the referee."""
    f_func = lambdify(m._symbolic_args, m.F_array.tolist(), modules=EXACT)
    j_func = lambdify(m._symbolic_args, m._J_sparse_array.tolist(), modules=EXACT)
    fields, pars = order_state()

    def F(U):
        return ora.compute_F(m, f_func, fields["x"], U, pars["k"], True, faithful_interleave=False)

    def J(U):
        return np.asarray(ora.compute_J(m, j_func, fields["x"], U, pars["k"], True).todense())
    return F, J


def backward_euler(m, dt):
    """The converged Newton solution of U1 = U0 + dt F(U1) (residual below 1e-15 in the max norm)."""
    F, J = dense_FJ(m)
    U0 = order_state()[0]["U"]
    U = U0.copy()
    for _ in range(30):
        r = U - U0 - dt * F(U)
        if np.abs(r).max() < 1e-15:
            return U
        U = U - np.linalg.solve(np.eye(U.size) - dt * J(U), r)
    raise AssertionError("Newton did not converge: residual %.3g" % np.abs(r).max())


def theta_errors(backend, dts=ORDER_DTS):
    """{mode: [max-norm error of one linearised backward-Euler step against the Newton solution per dt]}."""
    ref = {dt: backward_euler(model("burgers_up", "exact", oracle=True), dt) for dt in dts}
    out = {}
    for mode in ("exact", "one"):
        m = model("burgers_up", mode, backend)
        fields, pars = order_state()
        errs = []
        for dt in dts:
            _, f = schemes.Theta(m, theta=1)(0.0, m.fields_template(**fields), dt, pars)
            errs.append(float(np.abs(np.asarray(f.uflat) - ref[dt]).max()))
        out[mode] = errs
    return out


def check_step_order(backend, dts=ORDER_DTS):
    errs = theta_errors(backend, dts)
    for dt, e, o in zip(dts, errs["exact"], errs["one"]):
        print("dt = %.0e: error with the exact J %.3e, with Heaviside == 1 %.3e (1/%.0f)" % (dt, e, o, o / e))
    for a, b in zip(errs["exact"], errs["exact"][1:]):
        assert a / b >= 6.0, errs                   # third order: 8
    for e, o in zip(errs["exact"], errs["one"]):
        assert e <= o / 20.0, errs


# ---------------------------------------------------------------------------------- observers
#: the carrier of the observer cases: Burgers with a scalar or per-node parameter c that only the
#: observers read, through the model's parameter slots
OBS_MODEL = ("k*dxxU - upwind(U, U, 2)", "U", ["k", "c"])
OBS_STEP = "Heaviside(U - c) * U"
OBS_PIECE = "Piecewise((U, U > 0), (0, True))"
OBS_RIGHT = "Heaviside(U)"
OBS_C = 0.5


def observer_model(mode="exact", compiled=True):
    key = ("observer", mode, compiled)
    if key not in _CACHE:
        _CACHE[key] = Model(*OBS_MODEL, heaviside=mode, hold_compilation=not compiled)
    return _CACHE[key]


def observer_inputs(N, periodic, per_node, member=0):
    """(fields, pars, dt): a smooth state that crosses zero and c, with exact zeros of both signs and exact
    ties U = c at t0."""
    x = np.linspace(0.0, 1.0, N, endpoint=not periodic)
    U = np.sin(2 * np.pi * x) * (1.0 + 0.1 * member) + 0.2
    c = OBS_C + 0.1 * np.cos(2 * np.pi * x) if per_node else np.float64(OBS_C + 0.05 * member)
    for i, v in ((3, 0.0), (6, -0.0), (9, _up(0.0)), (12, _down(0.0))):
        U[i] = v
    U[15] = c[15] if per_node else c
    U[18] = _up(U[15])
    U[21] = _down(U[15])
    return dict(x=x, U=U), dict(k=1e-3, c=c, periodic=periodic), 1e-4


OBS_MODES = [0, 1, 2, 5]
OBS_STEPS = 3


def add_observers(front):
    """The five observers of the cases on a Simulation or an Ensemble."""
    front.add_probe("right", OBS_RIGHT, reduce="integral")
    front.add_recorder("positive", OBS_PIECE)
    front.add_statistic("gated", OBS_STEP, stat="mean")
    front.add_spectrum("amps", OBS_STEP, modes=OBS_MODES)
    front.add_extrema("crests", OBS_STEP)


def check_observers(m, got, states, pars, periodic, label=""):
    """One system's series (``got``: dict of probes, recorders, statistics, spectra, extrema) against the
    NumPy reference on ``states = [(t, fields), ...]``: bits, but for the spectrum (its bound of DESIGN.md
    section 18)."""
    import math
    from tests import extrema_cases, spectrum_cases
    from tests.test_statistics import numpy_fold, value_of
    nodes = [numpy_nodes(m, [OBS_RIGHT, OBS_PIECE, OBS_STEP], f, pars) for _, f in states]
    x = np.asarray(states[0][1]["x"])
    N = x.size
    dx = (x[-1] - x[0]) / (N - 1)
    times = np.array([t for t, _ in states])
    t, v = got["probes"]["right"]
    want = []
    for nd in nodes:
        s = math.fsum(nd[0])                          # (multiples of 1/2: every order of the sum is exact)
        want.append(dx * s if periodic else dx * (s - (nd[0][0] + nd[0][-1]) / 2))
    assert np.array_equal(t, times) and np.array_equal(v, np.array(want)), (label, v, want)
    assert 0.0 < v[0] < 1.0
    t, xs, values = got["recorders"]["positive"]
    assert np.array_equal(t, times) and np.array_equal(xs, x), label
    assert same_bits(values, np.array([nd[1] for nd in nodes])), label
    n, xs, values = got["statistics"]["gated"]
    samples = [(tt, nd[2]) for tt, nd in zip(times, nodes)]
    assert n == len(states) and same_bits(values, value_of("mean", numpy_fold("mean", samples), n)), label
    t, k, c = got["spectra"]["amps"]
    r = spectrum_cases.ratios(c, np.array([nd[2] for nd in nodes]), OBS_MODES)
    print("%s spectrum: worst |c - c_ref| / (2**-53 sum|v|) = %.3f" % (label, r.max()))
    assert np.array_equal(t, times) and (r <= spectrum_cases.BOUND_ULPS).all(), (label, r.max())
    t, n, g, xs, vs = got["extrema"]["crests"]
    assert np.array_equal(t, times), label
    for row, nd in enumerate(nodes):
        extrema_cases.assert_row((n[row], g[row], xs[row], vs[row]), nd[2], x, "max", periodic, None, 256, True,
                                 label=(label, row))
    assert n.min() >= 1, (label, n)


def check_simulation_observers(N, periodic, per_node):
    from triflow_amd.simulation import Simulation
    m = observer_model("exact")
    fields, pars, dt = observer_inputs(N, periodic, per_node)

    def run(observed):
        sim = Simulation(m, dict(fields), dict(pars), dt=dt, scheme=schemes.ROS2, time_stepping=False)
        if observed:
            add_observers(sim)
        states = [(sim.t, dict(x=fields["x"], U=np.array(sim.fields["U"])))]
        for _ in range(OBS_STEPS):
            t, f = next(sim)
            states.append((t, dict(x=fields["x"], U=np.array(f["U"]))))
        return sim, states
    sim, _ = run(True)
    got = dict(probes=sim.probes, recorders=sim.recorders, statistics=sim.statistics, spectra=sim.spectra,
               extrema=sim.extrema)
    _, states = run(False)                            # (the steps are bitwise deterministic)
    check_observers(m, got, states, pars, periodic, label="N=%d %s %s" % (
        N, "periodic" if periodic else "clamped", "per-node c" if per_node else "scalar c"))


def check_ensemble_observers(N=1031, nsys=3):
    from triflow_amd.ensemble import Ensemble
    m = observer_model("exact")
    members = [observer_inputs(N, True, False, member=e) for e in range(nsys)]
    x, dt = members[0][0]["x"], members[0][2]
    member_pars = dict(k=1e-3, c=np.array([p["c"] for _, p, _ in members]), periodic=True)
    ens = Ensemble(m, x, dict(U=np.array([f["U"] for f, _, _ in members])), member_pars, periodic=True, scheme="ROS2")
    add_observers(ens)
    states = [(ens.t, ens.state())]
    for _ in range(OBS_STEPS):
        ens.step(dt)
        states.append((ens.t, ens.state()))
    got = dict(probes=ens.probes, recorders=ens.recorders, statistics=ens.statistics, spectra=ens.spectra,
               extrema=ens.extrema)
    ens.close()
    for e in range(nsys):
        mine = dict(probes={k: (t, v[:, e]) for k, (t, v) in got["probes"].items()},
                    recorders={k: (t, xs, v[:, e]) for k, (t, xs, v) in got["recorders"].items()},
                    statistics={k: (n, xs, v[e]) for k, (n, xs, v) in got["statistics"].items()},
                    spectra={k: (t, kk, c[:, e]) for k, (t, kk, c) in got["spectra"].items()},
                    extrema={k: (s[0],) + tuple(a[:, e] for a in s[1:]) for k, s in got["extrema"].items()})
        pe = dict(k=1e-3, c=member_pars["c"][e], periodic=True)
        check_observers(m, mine, [(t, dict(x=x, U=st[0, e])) for t, st in states], pe, True, label="member %d" % e)


def check_default_mode_observers_refuse():
    import pytest
    from triflow_amd.codegen import UnsupportedExpression
    from triflow_amd.simulation import Simulation
    m = observer_model("one")
    fields, pars, dt = observer_inputs(50, True, False)
    sim = Simulation(m, fields, pars, dt=dt, scheme=schemes.ROS2, time_stepping=False)
    for call in (lambda: sim.add_probe("right", OBS_RIGHT, reduce="integral"),
                 lambda: sim.add_recorder("positive", OBS_PIECE),
                 lambda: sim.add_statistic("gated", OBS_STEP, stat="mean"),
                 lambda: sim.add_spectrum("amps", OBS_STEP, modes=OBS_MODES),
                 lambda: sim.add_extrema("crests", OBS_STEP)):
        with pytest.raises(UnsupportedExpression, match="Heaviside|select"):
            call()
    assert sim.probes == {} and sim.recorders == {} and sim.statistics == {} and sim.spectra == {} \
        and sim.extrema == {}
    next(sim)                                         # the run goes on unobserved


def check_uniform_planes_follow_a_scalar(backend):
    """Heaviside(c) * dxU: every entry is node-independent, evaluated on the device and written by the
    first F+J sweep after an upload of c only; J read back is that of the c uploaded last."""
    key = ("uniform", id(backend))
    if key not in _CACHE:
        compiler = hip_compiler if backend is None else partial(hip_compiler, backend=backend)
        _CACHE[key] = Model("k*dxxU - Heaviside(c)*dxU", "U", ["k", "c"], compiler=compiler, heaviside="exact")
    m = _CACHE[key]
    cm = m._device
    N = 1031
    x = np.linspace(0.0, 1.0, N)
    U = np.cos(5 * x)
    s = cm.solver(N, False, 1, 0)
    assert s.model.spec["j_uniform"] == [1, 1, 1]
    cm.bind_inputs(s, x, [1e-3, 0.75], None)
    s.set_state(0, np.array([U]))
    start = s.jacobian_sweeps()
    fulls, corner = [], []
    for upload in (None, None, -0.75, 0.0):
        if upload is not None:
            s.set_param(1, float(upload))
        c = 0.75 if upload is None else upload
        s.eval(0, with_j=True)
        s.eval(0, with_j=True)
        J = np.array(s.get_J()[0]).reshape(N, -1).T
        _, Jn = numpy_FJ(m, dict(x=x, U=U), dict(k=1e-3, c=c, periodic=False))
        assert same_bits(J, Jn), c
        sw = s.jacobian_sweeps()
        fulls.append(sw["full"] - start["full"])
        corner.append(J[0, 5])
        assert sw["full"] + sw["lean"] - start["full"] - start["lean"] == 2 * len(fulls), sw
    # one full-table sweep after the first upload, none while c stays, one after each change of c
    assert fulls == [1, 1, 2, 3], fulls
    assert corner[0] == corner[1] and len(set(corner)) == 3, corner          # H(c) = 1, 1, 0, 1/2


# ---------------------------------------------------------------------------------- observers on the host
def stepped_states(backend, N, periodic, per_node):
    """[(t, fields)]: the initial state of the observer cases and the states after OBS_STEPS steps of ROS2
    of the exact-mode model on ``backend`` (the CPU tier: the emulation), with their parameters."""
    from triflow_amd.simulation import Simulation
    key = ("observer", id(backend))
    if key not in _CACHE:
        _CACHE[key] = Model(*OBS_MODEL, heaviside="exact", compiler=partial(hip_compiler, backend=backend))
    fields, pars, dt = observer_inputs(N, periodic, per_node)
    sim = Simulation(_CACHE[key], dict(fields), dict(pars), dt=dt, scheme=schemes.ROS2, time_stepping=False)
    states = [(sim.t, dict(x=fields["x"], U=np.array(sim.fields["U"])))]
    for _ in range(OBS_STEPS):
        t, f = next(sim)
        states.append((t, dict(x=fields["x"], U=np.array(f["U"]))))
    return states, pars


def check_observers_on_the_host(states, pars, periodic, P, per_node):
    """The five observers of the cases through their host harnesses (the generated block and
    csrc/tf_probe.h, tf_record.h, tf_stat.h, tf_spectrum.h, tf_extrema.h compiled with g++) on ``states``
    against the NumPy reference: bits, but for the spectrum (its bound of DESIGN.md section 18)."""
    import math
    from tests import extrema_cases, spectrum_cases
    from tests.extrema_host import build_extrema_host as ehost
    from tests.probe_host import build_probe_host as phost
    from tests.record_host import build_record_host as rhost
    from tests.spectrum_host import build_spectrum_host as shost
    from tests.stat_host import build_stat_host as sthost
    from tests.test_statistics import numpy_fold
    m = observer_model("exact", compiled=False)
    mask = 2 if per_node else 0
    x = states[0][1]["x"]
    N = x.size
    dx = (x[-1] - x[0]) / (N - 1)
    label = (N, periodic, per_node)
    nodes = [numpy_nodes(m, [OBS_RIGHT, OBS_PIECE, OBS_STEP], f, pars) for _, f in states]
    stat = sthost.Harness(m, [OBS_STEP], x, pars, periodic, P, mask)
    spec = shost.Harness(m, [OBS_STEP], x, pars, periodic, P, mask)
    ext = ehost.Harness(m, [OBS_STEP], x, pars, periodic, P, mask)
    acc = stat.planes("mean")
    for k, ((t, f), nd) in enumerate(zip(states, nodes), 1):
        only_u = dict(U=f["U"])
        got_nodes, got = phost.run(m, [OBS_RIGHT], ["integral"], x, only_u, pars, periodic, P, mask)
        s = math.fsum(nd[0])                          # (multiples of 1/2: every order of the sum is exact)
        want = dx * s if periodic else dx * (s - (nd[0][0] + nd[0][-1]) / 2)
        assert same_bits(got_nodes[0], nd[0]) and got[0] == want, (label, k, got[0], want)
        row = rhost.Harness(m, [OBS_PIECE], x, only_u, pars, periodic, P, mask).row(0, "sample", slice(None))
        assert same_bits(row, nd[1]), (label, k)
        stat.update(0, "mean", k, t, stat.state(only_u), acc)
        want = numpy_fold("mean", [(tt, n2[2]) for (tt, _), n2 in zip(states[:k], nodes[:k])])
        assert same_bits(stat.natural(acc), want), (label, k)
        r = spectrum_cases.ratios(spec.run(0, OBS_MODES, only_u), nd[2], OBS_MODES)
        assert (r <= spectrum_cases.BOUND_ULPS).all(), (label, k, r.max())
        n, g, triples = ext.run(0, only_u, "max")
        rg, rt = extrema_cases.referee(nd[2], "max", periodic, None)
        assert n == rg.size >= 1 and np.array_equal(g, rg) and same_bits(triples, rt), (label, k, n, rg.size)
    assert 0.0 < want.max() and len(states) == OBS_STEPS + 1
