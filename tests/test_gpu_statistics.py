"""Device statistics on the MI355X: the accumulators against the recurrences in NumPy on the same states,
graph replay, bitwise reproducibility, residency of the state, reset, adaptive steps, ensembles, probes,
recorders and statistics together, a change of solver in the middle of a run."""
import numpy as np
import pytest

from tests.test_gpu_recorders import _ensemble_case, film_inputs, m1_inputs, model_of, simulation, states_of
from tests.test_statistics import numpy_fold, numpy_nodes, value_of
from triflow_amd import Simulation
from triflow_amd._capi import DeviceSolver, DeviceStat
from triflow_amd.ensemble import Ensemble

pytestmark = pytest.mark.gpu

WINDOW = slice(2001, 60000, 100)
# (name, expression, keywords of add_statistic): two expressions, all six kinds, every 1 and 3, a window.
# The statistics of the first expression come first: the sets of the tests share their code objects.  (No
# cube of a node value: DESIGN.md section 15.)
FILM_STATS = [("hbar", "h", dict(stat="mean")),
              ("hvar", "h", dict(stat="var", every=3)),
              ("env", "h", dict(stat="max")),
              ("low", "h", dict(stat="min", every=3, nodes=WINDOW)),
              ("when", "We * h * dxxxh", dict(stat="argmax")),
              ("whenlow", "We * h * dxxxh", dict(stat="argmin", every=3)),
              ("fvar", "We * h * dxxxh", dict(stat="var", nodes=WINDOW)),
              ("fbar", "We * h * dxxxh", dict(stat="mean", every=3))]
M1_STATS = [("ubar", "U", dict(stat="mean", every=3)),
            ("uvar", "U", dict(stat="var")),
            ("top", "U", dict(stat="max", every=3)),
            ("low", "U", dict(stat="min")),
            ("when", "c * dxU**2", dict(stat="argmax", every=3, nodes=WINDOW)),
            ("whenlow", "c * dxU**2", dict(stat="argmin")),
            ("gvar", "c * dxU**2", dict(stat="var", every=3)),
            ("gbar", "c * dxU**2", dict(stat="mean", nodes=WINDOW))]


def run_with(inputs, stats, steps):
    sim = simulation(inputs)
    for name, expr, kw in stats:
        sim.add_statistic(name, expr, **kw)
    for _ in range(steps):
        next(sim)
    return sim


def assert_statistics(model, stats, got, states, pars, first=None):
    """``got`` (a front end's ``statistics``) against the NumPy fold of ``states = [(t, fields), ...]``;
    ``pars``: the parameters, or one dict per state; ``first``: per statistic, the index of the state
    of sample 1 (default 0)."""
    exprs = []
    for _, e, _ in stats:
        if e not in exprs:
            exprs.append(e)
    per_state = pars if isinstance(pars, list) else [pars] * len(states)
    nodes = [numpy_nodes(model, exprs, f, p) for (_, f), p in zip(states, per_state)]
    x = np.asarray(states[0][1]["x"])
    for name, e, kw in stats:
        kind, window = kw.get("stat", "mean"), kw.get("nodes", slice(None))
        idx = range((first or {}).get(name, 0), len(states), kw.get("every", 1))
        samples = [(states[i][0], nodes[i][exprs.index(e)]) for i in idx]
        want = value_of(kind, numpy_fold(kind, samples), len(samples))[window]
        n, xs, values = got[name]
        assert n == len(samples), (name, n)
        assert np.array_equal(xs, x[window]) and values.shape == want.shape, name
        assert values.tobytes() == want.tobytes(), (name, np.nanmax(np.abs(values - want)))


@pytest.mark.parametrize("inputs,stats", [(film_inputs(100003), FILM_STATS), (m1_inputs(20011), M1_STATS)],
                         ids=["film-ragged", "M1-clamped-ragged"])
def test_statistics_match_numpy_on_the_same_states(inputs, stats):
    steps = 12
    got = run_with(inputs, stats, steps).statistics
    states = states_of(inputs, steps)
    assert_statistics(model_of(inputs[0]), stats, got, states, inputs[2])
    assert sorted({got[name][0] for name, _, _ in stats}) == [5, 13]          # every 3rd state, every state


def test_small_grid_with_graph_replay():
    """Config 3 at 20 000 nodes (graph replay on by default below 5e4 nodes): the number of the sample and
    its time are arguments of the launch, and a replayed step must not freeze them."""
    inputs = film_inputs(20_000)
    stats = [FILM_STATS[0], FILM_STATS[4]]
    steps = 30
    got = run_with(inputs, stats, steps).statistics
    states = states_of(inputs, steps)
    assert_statistics(model_of(inputs[0]), stats, got, states, inputs[2])
    assert got["hbar"][0] == steps + 1
    assert np.unique(got["when"][2]).size > 1


def test_two_runs_are_bit_identical():
    inputs = film_inputs(100003)
    one, two = run_with(inputs, FILM_STATS, 9).statistics, run_with(inputs, FILM_STATS, 9).statistics
    for name, _, _ in FILM_STATS:
        assert one[name][0] == two[name][0] and one[name][2].tobytes() == two[name][2].tobytes(), name


def test_state_stays_resident(monkeypatch):
    calls = dict(up=0, down=0, fetch=0, doubles=0)
    for meth, key in (("set_state", "up"), ("get_state", "down"), ("get_state_flat", "down")):
        orig = getattr(DeviceSolver, meth)

        def counted(self, *a, _orig=orig, _key=key, **k):
            calls[_key] += 1
            return _orig(self, *a, **k)
        monkeypatch.setattr(DeviceSolver, meth, counted)
    orig_fetch = DeviceStat.fetch

    def fetch(self, which):
        out = orig_fetch(self, which)
        calls["fetch"] += 1
        calls["doubles"] += out.size
        return out
    monkeypatch.setattr(DeviceStat, "fetch", fetch)
    N = 200_000
    inputs = film_inputs(N)
    sim = simulation(inputs)
    for name, expr, kw in FILM_STATS[:2]:
        sim.add_statistic(name, expr, **kw)
    # (the initial state is a host container: every add_statistic before the first step uploads it for
    # its sample 1, as add_probe does; the run itself starts here)
    calls.update(up=0, down=0, fetch=0, doubles=0)
    for _ in range(60):
        t, f = next(sim)
        assert f._device_backing() is not None and f._device_backing().valid()
    assert calls == dict(up=1, down=0, fetch=0, doubles=0), calls
    got = sim.statistics
    assert calls == dict(up=1, down=0, fetch=2, doubles=3 * N), calls        # mean: one plane, var: two
    assert got["hbar"][0] == 61 and got["hvar"][0] == 21 and got["hbar"][2].shape == (N,)


def test_reset_drops_the_transient():
    inputs = film_inputs(4096)
    stats = FILM_STATS[:5]
    sim = run_with(inputs, stats, 5)
    for name in ("hbar", "hvar", "when"):
        sim.reset_statistic(name)
    assert sim.statistics["hbar"][0] == 0 and np.isnan(sim.statistics["hbar"][2]).all()
    for _ in range(7):
        next(sim)
    got = sim.statistics
    states = states_of(inputs, 12)
    assert got["hbar"][0] == 7 and got["when"][0] == 7 and got["hvar"][0] == 3 and got["env"][0] == 13
    assert_statistics(model_of(inputs[0]), stats, got, states, inputs[2], first=dict(hbar=6, hvar=6, when=6))


def test_adaptive_default_scheme():
    inputs = film_inputs(4096)
    name, fields, pars = inputs[:3]
    stats = [FILM_STATS[0], FILM_STATS[2], FILM_STATS[4]]
    sim = Simulation(model_of(name), fields, pars, dt=1e-2)          # the default scheme, time_stepping=True
    for sname, expr, kw in stats:
        sim.add_statistic(sname, expr, **kw)
    keys = ["x", *model_of(name)._dep_vars]
    states = [(sim.t, {k: np.array(sim.fields[k]) for k in keys})]
    sim.add_post_process("keep", lambda s: states.append((s.t, {k: np.array(s.fields[k]) for k in keys})))
    states.pop()                                                     # (add_post_process ran it once)
    for _ in range(6):
        next(sim)
    got = sim.statistics
    assert len(states) == 7 and got["hbar"][0] == 7
    assert_statistics(model_of(name), stats, got, states, pars)


def test_ensemble_members():
    model, fields, fdict, member_pars, dt = _ensemble_case()
    nsys = 8
    stats = [FILM_STATS[0], FILM_STATS[1], FILM_STATS[4],
             ("fvar", "We * h * dxxxh", dict(stat="var", nodes=slice(1, 4000, 100)))]
    ens = Ensemble(model, fields["x"], fdict, member_pars, periodic=True, scheme="ROS2")
    for name, expr, kw in stats:
        ens.add_statistic(name, expr, **kw)
    states = [(ens.t, ens.state())]
    for _ in range(9):
        ens.step(dt)
        states.append((ens.t, ens.state()))
    got = ens.statistics
    ens.close()
    assert got["hbar"][2].shape == (nsys, 4096) and got["fvar"][2].shape == (nsys, 40)
    assert got["hbar"][1].shape == (4096,) and got["hvar"][0] == 4
    for e in range(nsys):
        pe = {k: (v[e] if np.ndim(v) else v) for k, v in member_pars.items()}
        mine = [(t, dict(x=fields["x"], **{k: st[j, e] for j, k in enumerate(model._dep_vars)})) for t, st in states]
        assert_statistics(model, stats, {k: (n, x, v[e]) for k, (n, x, v) in got.items()}, mine, pe)


def test_with_probes_and_recorders_together():
    inputs = film_inputs(100003)

    def run(with_statistic):
        sim = simulation(inputs)
        sim.add_probe("mass", "h", reduce="integral")
        sim.add_recorder("crest", "h", every=3, nodes=slice(None, None, 64), pool="max")
        if with_statistic:
            sim.add_statistic(*FILM_STATS[1][:2], **FILM_STATS[1][2])
        for _ in range(10):
            next(sim)
        return sim.probes, sim.recorders, sim.statistics
    p1, r1, s1 = run(True)
    p0, r0, _ = run(False)
    assert np.array_equal(p1["mass"][0], p0["mass"][0]) and p1["mass"][1].tobytes() == p0["mass"][1].tobytes()
    assert np.array_equal(r1["crest"][0], r0["crest"][0]) and r1["crest"][2].tobytes() == r0["crest"][2].tobytes()
    assert p1["mass"][1].shape == (11,) and r1["crest"][2].shape[0] == 4 and s1["hvar"][0] == 4
    assert (s1["hvar"][2] >= 0).all() and s1["hvar"][2].max() > 0


def test_solver_change_keeps_the_samples():
    """A Python hook hands the run a per-node parameter after step 4 of 8: the next step runs on the solver
    of that parameter layout, and the statistics go on there with the accumulators of the first."""
    inputs = film_inputs(4096)
    name, fields, pars, dt, _ = inputs
    model = model_of(name)
    x = np.asarray(fields["x"])
    stats = [FILM_STATS[0], FILM_STATS[1], FILM_STATS[4]]

    def hook(t, f, p):
        if t > 3.5 * dt and np.ndim(p["We"]) == 0:
            f["h"] = np.array(f["h"])            # (a host container again: the step binds a solver for it)
            p = dict(p, We=p["We"] * (1.0 + 0.25 * np.cos(2 * np.pi * x / (x[-1] + x[1]))))
        return f, p

    def run(with_statistics):
        sim = simulation((name, fields, pars, dt, hook))
        if with_statistics:
            for sname, expr, kw in stats:
                sim.add_statistic(sname, expr, **kw)
        keys = ["x", *model._dep_vars]
        states, used = [(sim.t, {k: np.array(sim.fields[k]) for k in keys})], [dict(sim.parameters)]
        for _ in range(8):
            t, f = next(sim)
            if not with_statistics:
                states.append((t, {k: np.array(f[k]) for k in keys}))
                used.append(dict(sim.parameters))
        return sim, states, used
    sim, _, _ = run(True)
    got = sim.statistics
    assert len(sim._statistics._bound) == 2                          # two solvers, one handle each
    _, states, used = run(False)
    assert np.ndim(used[4]["We"]) == 0 and np.ndim(used[5]["We"]) == 1
    assert got["hbar"][0] == 9 and got["when"][0] == 9 and got["hvar"][0] == 3
    assert_statistics(model, stats, got, states, used)
