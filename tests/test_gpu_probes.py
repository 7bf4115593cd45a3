"""Device probes on the MI355X: values against NumPy on the same states, bitwise reproducibility,
residency of the state, the default Simulation path, graph replay, ensembles."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
from sympy import lambdify

from oracle import numpy_path as ora
from triflow_amd import Model, Simulation, probes, schemes, workloads
from triflow_amd._capi import DeviceProbe, DeviceSolver
from triflow_amd.ensemble import Ensemble

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FILM_PROBES = [("mass", "h", "integral"), ("crest", "h", "max"), ("where", "h", "argmax"),
               ("slope", "We**3 * dxh**2", "mean")]
M1_PROBES = [("mass", "U", "integral"), ("low", "U", "min"), ("where", "U * x", "argmin"),
             ("grad", "c * dxU**2", "sum")]

_MODELS = {}


def model_of(name):
    if name not in _MODELS:
        _MODELS[name] = Model(*workloads.model_args(name))
    return _MODELS[name]


def film_inputs(N):
    _, fields, pars, dt, _ = workloads.config_inputs(3, N)
    return "M3_film", fields, pars, dt


def m1_inputs(N):
    x = np.linspace(0, 1, N)
    return "M1_advdiff", dict(x=x, U=np.cos(2 * np.pi * x * 5) + x), dict(c=.03, k=.001, periodic=False), 1e-3


def reference_row(model, probe_list, fields, pars):
    """The probes of one downloaded state, in NumPy: the lambdified discretised expressions with the
    reference's module dictionary on the ghost-padded views, then the reductions."""
    disc = [probes.discretise(model, p[1]) for p in probe_list]
    func = lambdify(model._symbolic_args, disc, modules=ora._lambdify_modules())
    inputs = [np.asarray(fields["x"])] + [np.asarray(fields[k]) for k in model._dep_vars] + \
        [pars[k] for k in model._pars] + [pars["periodic"]]
    env, N, _, periodic = ora.stencil_views(model, *inputs)
    vals = func(*[env[k] for k in model._args])
    x = np.asarray(fields["x"])
    dx = (x[-1] - x[0]) / (N - 1)
    out = []
    for (_, _, kind), v in zip(probe_list, vals):
        f = np.broadcast_to(np.asarray(v, dtype=float), (N,))
        s = math.fsum(f)
        ref = {"sum": lambda: s, "mean": lambda: s / N,
               "integral": lambda: dx * s if periodic else dx * (s - (f[0] + f[-1]) / 2),
               "max": lambda: np.max(f), "min": lambda: np.min(f),
               "argmax": lambda: x[np.argmax(f)], "argmin": lambda: x[np.argmin(f)]}[kind]()
        scale = math.fsum(np.abs(f)) * {"integral": dx, "mean": 1.0 / N}.get(kind, 1.0)
        out.append((ref, scale))
    return out


def assert_row_matches(kind_list, got, ref):
    for kind, g, (r, scale) in zip(kind_list, got, ref):
        if kind in ("sum", "mean", "integral"):
            assert abs(g - r) <= 1e-14 * scale, (kind, g, r)
        else:
            assert g == r, (kind, g, r)


def probed_run(inputs, probe_list, steps, scheme=schemes.ROS2):
    name, fields, pars, dt = inputs
    sim = Simulation(model_of(name), fields, pars, dt=dt, scheme=scheme, time_stepping=False)
    for pname, expr, kind in probe_list:
        sim.add_probe(pname, expr, reduce=kind)
    for _ in range(steps):
        next(sim)
    return sim.probes


@pytest.mark.parametrize("inputs", [film_inputs(10 ** 6), film_inputs(100003), m1_inputs(20011)],
                         ids=["film-1e6", "film-ragged", "M1-clamped-ragged"])
def test_probes_match_numpy_on_the_same_states(inputs):
    name = inputs[0]
    probe_list = FILM_PROBES if name == "M3_film" else M1_PROBES
    steps = 20
    got = probed_run(inputs, probe_list, steps)
    # the same run again, its state downloaded after every step (the steps are bitwise deterministic)
    model = model_of(name)
    _, fields, pars, dt = inputs
    sim = Simulation(model, fields, pars, dt=dt, scheme=schemes.ROS2, time_stepping=False)
    keys = ["x", *model._dep_vars]
    states = [(sim.t, {k: np.array(sim.fields[k]) for k in keys})]
    for _ in range(steps):
        t, f = next(sim)
        states.append((t, {k: np.array(f[k]) for k in keys}))
    kinds = [p[2] for p in probe_list]
    for row, (t, state) in enumerate(states):
        ref = reference_row(model, probe_list, state, pars)
        vals = [got[p[0]][1][row] for p in probe_list]
        assert all(got[p[0]][0][row] == t for p in probe_list)
        assert_row_matches(kinds, vals, ref)
    assert all(got[p[0]][1].shape == (steps + 1,) for p in probe_list)


def test_two_runs_are_bit_identical():
    a = probed_run(film_inputs(10 ** 6), FILM_PROBES, 20)
    b = probed_run(film_inputs(10 ** 6), FILM_PROBES, 20)
    for p in FILM_PROBES:
        assert np.array_equal(a[p[0]][0], b[p[0]][0])
        assert a[p[0]][1].tobytes() == b[p[0]][1].tobytes(), p[0]


def test_state_stays_resident(monkeypatch):
    calls = {"get": 0, "fetch": 0}
    for meth in ("get_state", "get_state_flat"):
        orig = getattr(DeviceSolver, meth)

        def counted(self, *a, _orig=orig, **k):
            calls["get"] += 1
            return _orig(self, *a, **k)
        monkeypatch.setattr(DeviceSolver, meth, counted)
    orig_fetch = DeviceProbe.fetch

    def fetch(self):
        calls["fetch"] += 1
        return orig_fetch(self)
    monkeypatch.setattr(DeviceProbe, "fetch", fetch)
    monkeypatch.setattr(probes, "DEFAULT_CAPACITY", 64)
    name, fields, pars, dt = film_inputs(200_000)
    sim = Simulation(model_of(name), fields, pars, dt=dt, scheme=schemes.ROS2, time_stepping=False)
    for pname, expr, kind in FILM_PROBES[:3]:
        sim.add_probe(pname, expr, reduce=kind)
    for _ in range(200):
        t, f = next(sim)
        assert f._device_backing() is not None and f._device_backing().valid()
    assert calls["get"] == 0
    series = sim.probes
    assert calls["get"] == 0
    assert calls["fetch"] <= math.ceil(201 / 64) + 1
    assert all(series[p[0]][1].shape == (201,) for p in FILM_PROBES[:3])
    # the ring was drained three times on the way: same rows as a run with the default ring
    monkeypatch.setattr(probes, "DEFAULT_CAPACITY", 1024)
    sim2 = Simulation(model_of(name), fields, pars, dt=dt, scheme=schemes.ROS2, time_stepping=False)
    for pname, expr, kind in FILM_PROBES[:3]:
        sim2.add_probe(pname, expr, reduce=kind)
    for _ in range(200):
        next(sim2)
    for p in FILM_PROBES[:3]:
        assert sim2.probes[p[0]][1].tobytes() == series[p[0]][1].tobytes()


def test_default_simulation_records_every_yield():
    name, fields, pars, _ = film_inputs(4096)
    sim = Simulation(model_of(name), fields, pars, dt=1e-2)          # RODASPR, time_stepping=True
    sim.add_probe("mass", "h", reduce="integral")
    sim.add_probe("crest", "h", reduce="max")
    times = [sim.t]
    for _ in range(5):
        t, _ = next(sim)
        times.append(t)
    for p in ("mass", "crest"):
        t, v = sim.probes[p]
        assert np.array_equal(t, np.array(times)) and v.shape == (6,)
    assert np.all(np.isfinite(sim.probes["mass"][1]))
    sim.remove_probe("crest")
    next(sim)
    assert list(sim.probes) == ["mass"] and sim.probes["mass"][1].shape == (7,)


def small_run(out_path):
    """Config 3 at 20 000 nodes (graph replay on by default below 5e4 nodes), 30 steps."""
    got = probed_run(film_inputs(20_000), FILM_PROBES, 30)
    np.savez(out_path, **{p[0]: got[p[0]][1] for p in FILM_PROBES})


def test_graph_replay_gives_the_same_rows(tmp_path):
    small_run(str(tmp_path / "graphs_on.npz"))
    env = dict(os.environ, TRIFLOW_GRAPHS="0")
    code = "import sys; from tests.test_gpu_probes import small_run; small_run(sys.argv[1])"
    res = subprocess.run([sys.executable, "-c", code, str(tmp_path / "graphs_off.npz")], cwd=ROOT, env=env,
                         capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    a, b = np.load(tmp_path / "graphs_on.npz"), np.load(tmp_path / "graphs_off.npz")
    for p in FILM_PROBES:
        assert a[p[0]].tobytes() == b[p[0]].tobytes(), p[0]


def test_ensemble_probes_per_member():
    name, fields, pars, dt = film_inputs(4096)
    nsys = 4
    model = model_of(name)
    member_pars = dict(pars)
    member_pars["We"] = np.array([.01, .02, .005, .015])
    member_pars["c"] = np.array([1., .5, 1.5, .8])
    fdict = {k: np.tile(fields[k], (nsys, 1)) for k in model._dep_vars}
    ens = Ensemble(model, fields["x"], fdict, member_pars, periodic=True, scheme="ROS2")
    for pname, expr, kind in FILM_PROBES:
        ens.add_probe(pname, expr, reduce=kind)
    states = [ens.state()]
    for _ in range(10):
        ens.step(dt)
        states.append(ens.state())
    for e in range(nsys):
        pe = {k: (v[e] if np.ndim(v) else v) for k, v in member_pars.items()}
        for row, st in enumerate(states):
            f = dict(x=fields["x"], **{k: st[j, e] for j, k in enumerate(model._dep_vars)})
            ref = reference_row(model, FILM_PROBES, f, pe)
            vals = [ens.probes[p[0]][1][row, e] for p in FILM_PROBES]
            assert_row_matches([p[2] for p in FILM_PROBES], vals, ref)
    assert ens.probes["mass"][1].shape == (11, nsys)
    ens.close()


def test_ring_of_four_rows_gives_the_rows_of_the_default_ring(monkeypatch):
    """50 rows through a ring of 4: the host counts the row, the full ring is drained twelve times on the
    way, and times and values are the bytes of the same run with the default ring (which never fills)."""
    default = probed_run(film_inputs(4096), FILM_PROBES, 49)
    monkeypatch.setattr(probes, "DEFAULT_CAPACITY", 4)
    small = probed_run(film_inputs(4096), FILM_PROBES, 49)
    for p in FILM_PROBES:
        assert small[p[0]][1].shape == (50,)
        assert small[p[0]][0].tobytes() == default[p[0]][0].tobytes(), p[0]
        assert small[p[0]][1].tobytes() == default[p[0]][1].tobytes(), p[0]


def ensemble_run(nsys, steps):
    name, fields, pars, dt = film_inputs(4096)
    model = model_of(name)
    member_pars = dict(pars)
    member_pars["We"] = np.linspace(.005, .02, nsys)
    member_pars["c"] = np.linspace(.5, 1.5, nsys)
    fdict = {k: np.tile(fields[k], (nsys, 1)) for k in model._dep_vars}
    ens = Ensemble(model, fields["x"], fdict, member_pars, periodic=True, scheme="ROS2")
    for pname, expr, kind in FILM_PROBES:
        ens.add_probe(pname, expr, reduce=kind)
    for _ in range(steps):
        ens.step(dt)
    got = dict(ens.probes)
    ens.close()
    return got


def test_ensemble_ring_of_four_rows_gives_the_rows_of_the_default_ring(monkeypatch):
    """Eight members, 10 rows [nsys][nprobe] through a ring of 4 (a workgroup of tfk_probe_final per
    member): byte-equal to the default ring, member by member -- a wrong row index or row stride shows."""
    default = ensemble_run(8, 9)
    monkeypatch.setattr(probes, "DEFAULT_CAPACITY", 4)
    small = ensemble_run(8, 9)
    for p in FILM_PROBES:
        assert small[p[0]][1].shape == (10, 8)
        assert np.asarray(small[p[0]][0]).tobytes() == np.asarray(default[p[0]][0]).tobytes(), p[0]
        assert small[p[0]][1].tobytes() == default[p[0]][1].tobytes(), p[0]
    # (the members differ: a row that landed in another member's place would show)
    assert len({small["crest"][1][-1, e] for e in range(8)}) == 8


def test_host_constants_follow_changed_parameters():
    """A DirichletHook that returns new parameters every step: the probes' host constants (We**3 of
    "slope") are refreshed with the parameters the step was bound with."""
    from triflow_amd.device import DirichletHook
    name, fields, pars, dt = film_inputs(4096)
    model = model_of(name)
    hook = DirichletHook(parameters=lambda t, p: {"We": 0.02 * (1.0 + 50.0 * t)})
    sim = Simulation(model, fields, pars, dt=dt, scheme=schemes.ROS2, time_stepping=False, hook=hook)
    for pname, expr, kind in FILM_PROBES:
        sim.add_probe(pname, expr, reduce=kind)
    keys = ["x", *model._dep_vars]
    seen = []
    # a post-process runs after the probes of a step: it sees the state and the parameters they saw
    sim.add_post_process("keep", lambda s: seen.append(
        (s.t, {k: np.array(s.fields[k]) for k in keys}, dict(s.parameters))))
    for _ in range(10):
        next(sim)
    got = sim.probes
    assert len({p["We"] for _, _, p in seen}) == 11
    for row, (t, state, p) in enumerate(seen):
        ref = reference_row(model, FILM_PROBES, state, p)
        vals = [got[q[0]][1][row] for q in FILM_PROBES]
        assert got["slope"][0][row] == t
        assert_row_matches([q[2] for q in FILM_PROBES], vals, ref)


def test_probe_added_mid_run_starts_then():
    name, fields, pars, dt = film_inputs(4096)
    sim = Simulation(model_of(name), fields, pars, dt=dt, scheme=schemes.ROS2, time_stepping=False)
    sim.add_probe("mass", "h", reduce="integral")
    for _ in range(5):
        next(sim)
    t_added = sim.t
    sim.add_probe("mass2", "h", reduce="integral")
    for _ in range(5):
        next(sim)
    t1, v1 = sim.probes["mass"]
    t2, v2 = sim.probes["mass2"]
    assert t1.shape == (11,) and t2.shape == (6,)
    assert t2[0] == t_added and np.array_equal(t2, t1[5:])
    assert v2.tobytes() == v1[5:].tobytes()
