"""Device spectra on the MI355X: the series against the extended-precision referee on the same states,
graph replay, bitwise reproducibility and the ring, residency of the state, the exact identities, ensembles,
the four kinds of observers together, a spectrum removed and a change of solver in the middle of a run,
adaptive steps."""
import numpy as np
import pytest

from tests import spectrum_cases as cases
from tests.test_gpu_recorders import _ensemble_case, film_inputs, m1_inputs, model_of, simulation, states_of
from tests.test_statistics import numpy_nodes
from triflow_amd import Simulation
from triflow_amd._capi import DeviceSolver, DeviceSpectrum
from triflow_amd.ensemble import Ensemble

pytestmark = pytest.mark.gpu

FILM_EXPRS = ("h", "We * h * dxxxh")
M1_EXPRS = ("U", "c * dxU**2")
WORST = dict(ratio=0.0)


def specs_of(exprs, N):
    """(name, expression, modes, every): two expressions, every 1 and 3, 32 low modes plus N // 4,
    N // 2 - 1 and N // 2."""
    modes = cases.low_and_top_modes(N)
    return [("a", exprs[0], modes, 1), ("b", exprs[1], modes, 3)]


def run_with(inputs, specs, steps, capacity=None, **kw):
    sim = simulation(inputs, **kw)
    for name, expr, modes, every in specs:
        sim.add_spectrum(name, expr, modes=modes, every=every, capacity=capacity)
    for _ in range(steps):
        next(sim)
    return sim


def assert_spectra(model, specs, got, states, pars, first=None, label=""):
    """``got`` (a front end's ``spectra``) against the referee on ``states = [(t, fields), ...]``; ``pars``:
    the parameters, or one dict per state; ``first``: per spectrum, the index of the state of its first
    row (default 0).  t, k and the row counts are exact, every mode of every row is within the bound."""
    exprs = []
    for _, e, _, _ in specs:
        if e not in exprs:
            exprs.append(e)
    per_state = pars if isinstance(pars, list) else [pars] * len(states)
    nodes = [numpy_nodes(model, exprs, f, p) for (_, f), p in zip(states, per_state)]
    x = np.asarray(states[0][1]["x"])
    N = x.size
    dx = (x[-1] - x[0]) / (N - 1)
    for name, e, modes, every in specs:
        idx = list(range((first or {}).get(name, 0), len(states), every))
        t, k, c = got[name]
        assert np.array_equal(t, np.array([states[i][0] for i in idx])), name
        assert np.array_equal(k, 2.0 * np.pi * np.asarray(modes, dtype=float) / (N * dx)), name
        assert c.shape == (len(idx), len(modes)) and c.dtype == np.complex128, (name, c.shape)
        v = np.array([nodes[i][exprs.index(e)] for i in idx])
        r = cases.ratios(c, v, modes)
        WORST["ratio"] = max(WORST["ratio"], float(r.max()))
        print("%s %s: worst |c - c_ref| / (2**-53 sum|v|) = %.3f (so far %.3f)" % (label, name, r.max(), WORST["ratio"]))
        assert (r <= cases.BOUND_ULPS).all(), (name, r.max())


@pytest.mark.parametrize("inputs,exprs", [(film_inputs(20011), FILM_EXPRS), (m1_inputs(100003), M1_EXPRS)],
                         ids=["film-ragged-replayed", "M1-clamped-ragged"])
def test_series_match_the_referee_on_the_same_states(inputs, exprs):
    steps = 12
    N = np.asarray(inputs[1]["x"]).size
    specs = specs_of(exprs, N)
    got = run_with(inputs, specs, steps).spectra
    states = states_of(inputs, steps)
    assert_spectra(model_of(inputs[0]), specs, got, states, inputs[2], label=inputs[0])
    assert got["a"][2].shape[0] == 13 and got["b"][2].shape[0] == 5


def test_small_grid_with_graph_replay():
    """Config 3 at 20 000 nodes (graph replay on by default below 5e4 nodes): the row index is an argument
    of the launch, and a replayed step must not freeze it or the slot."""
    inputs = film_inputs(20_000)
    steps = 30
    specs = [("a", "h", cases.low_and_top_modes(20_000), 1)]
    got = run_with(inputs, specs, steps).spectra
    assert_spectra(model_of(inputs[0]), specs, got, states_of(inputs, steps), inputs[2], label="replay")
    c = got["a"][2]
    assert c.shape[0] == steps + 1 and len({row.tobytes() for row in c}) == steps + 1


def test_two_runs_are_bit_identical_and_the_ring_wraps():
    inputs = film_inputs(20011)
    specs = specs_of(FILM_EXPRS, 20011)
    small = run_with(inputs, specs, 49, capacity=4).spectra          # 50 and 17 rows through 4
    whole = run_with(inputs, specs, 49).spectra
    again = run_with(inputs, specs, 49).spectra
    for name, _, _, every in specs:
        rows = len(range(0, 50, every))
        assert small[name][2].shape[0] == rows and np.array_equal(small[name][0], whole[name][0]), name
        assert small[name][2].tobytes() == whole[name][2].tobytes(), name
        assert again[name][2].tobytes() == whole[name][2].tobytes(), name
        assert len({row.tobytes() for row in small[name][2]}) == rows, name       # every row once


def test_state_stays_resident(monkeypatch):
    calls = dict(up=0, down=0, fetch=0, doubles=0)
    for meth, key in (("set_state", "up"), ("get_state", "down"), ("get_state_flat", "down")):
        orig = getattr(DeviceSolver, meth)

        def counted(self, *a, _orig=orig, _key=key, **k):
            calls[_key] += 1
            return _orig(self, *a, **k)
        monkeypatch.setattr(DeviceSolver, meth, counted)
    orig_fetch = DeviceSpectrum._fetch

    def fetch(self, ncols, *which):
        out = orig_fetch(self, ncols, *which)
        calls["fetch"] += 1
        calls["doubles"] += out.size
        return out
    monkeypatch.setattr(DeviceSpectrum, "_fetch", fetch)
    N = 200_000
    inputs = film_inputs(N)
    sim = simulation(inputs)
    sim.add_spectrum("a", "h", modes=range(33))
    sim.add_spectrum("b", "We * h * dxxxh", modes=[1, 2, 4, 8], every=3)
    # (the initial state is a host container: every add_spectrum before the first step uploads it for its
    # t0 row, as add_probe does; the second add fetched the t0 row of the first.  The run starts here)
    calls.update(up=0, down=0, fetch=0, doubles=0)
    for _ in range(60):
        t, f = next(sim)
        assert f._device_backing() is not None and f._device_backing().valid()
    assert calls == dict(up=1, down=0, fetch=0, doubles=0), calls
    got = sim.spectra
    assert got["a"][2].shape == (61, 33) and got["b"][2].shape == (21, 4)
    assert calls == dict(up=1, down=0, fetch=2, doubles=60 * 2 * 33 + 21 * 2 * 4), calls


def test_identities_on_the_device():
    inputs = film_inputs(20_000)
    N, steps = 20_000, 6
    sim = simulation(inputs)
    sim.add_spectrum("a", "h", modes=[0, 3, N // 4, N // 2])
    sim.add_spectrum("b", "We * h * dxxxh", modes=[N // 2, 0, 7])
    sim.add_probe("sum_h", "h", reduce="sum")
    for _ in range(steps):
        next(sim)
    (_, _, a), (_, _, b) = sim.spectra["a"], sim.spectra["b"]
    assert a.shape == (steps + 1, 4) and b.shape == (steps + 1, 3)
    assert (a[:, 0].imag == 0).all() and (b[:, 1].imag == 0).all()            # mode 0
    assert (a[:, 3].imag == 0).all() and (b[:, 0].imag == 0).all()            # mode N / 2 of an even N
    assert (a[:, 1].imag != 0).any() and (b[:, 2].imag != 0).any()
    _, total = sim.probes["sum_h"]
    states = states_of(inputs, steps)
    for i, (_, f) in enumerate(states):
        bound = cases.BOUND_ULPS * cases.UNIT * np.sum(np.abs(f["h"]))
        assert abs(a[i, 0].real - total[i]) <= bound, (i, a[i, 0].real - total[i], bound)


def test_ensemble_members():
    model, fields, fdict, member_pars, dt = _ensemble_case()
    nsys, N = 8, 4096
    specs = specs_of(FILM_EXPRS, N)
    ens = Ensemble(model, fields["x"], fdict, member_pars, periodic=True, scheme="ROS2")
    for name, expr, modes, every in specs:
        ens.add_spectrum(name, expr, modes=modes, every=every)
    states = [(ens.t, ens.state())]
    for _ in range(9):
        ens.step(dt)
        states.append((ens.t, ens.state()))
    got = ens.spectra
    ens.close()
    nm = len(specs[0][2])
    assert got["a"][2].shape == (10, nsys, nm) and got["b"][2].shape == (4, nsys, nm)
    assert got["a"][1].shape == (nm,)                                        # one grid for all members
    for e in range(nsys):
        pe = {k: (v[e] if np.ndim(v) else v) for k, v in member_pars.items()}
        mine = [(t, dict(x=fields["x"], **{k: st[j, e] for j, k in enumerate(model._dep_vars)})) for t, st in states]
        assert_spectra(model, specs, {k: (t, kk, c[:, e]) for k, (t, kk, c) in got.items()}, mine, pe,
                       label="member %d" % e)


def test_ensemble_members_with_grids_of_their_own():
    model, fields, fdict, member_pars, dt = _ensemble_case()
    x = np.asarray(fields["x"])
    xs = np.array([x * (1.0 + 0.125 * e) for e in range(8)])
    ens = Ensemble(model, xs, fdict, member_pars, periodic=True, scheme="ROS2")
    ens.add_spectrum("a", "h", modes=[0, 1, 2])
    ens.step(dt)
    t, k, c = ens.spectra["a"]
    ens.close()
    assert k.shape == (8, 3) and c.shape == (2, 8, 3)
    dxs = (xs[:, -1] - xs[:, 0]) / (x.size - 1)
    assert np.array_equal(k, 2.0 * np.pi * np.array([0., 1., 2.]) / (x.size * dxs[:, None]))


def test_with_the_other_observers_together_and_removed_mid_run():
    inputs = film_inputs(100003)
    N = 100003
    specs = [("a", "h", cases.low_and_top_modes(N, low=8), 1), ("b", "We * h * dxxxh", [1, 2, 4, 8], 2)]

    def run(with_spectra):
        sim = simulation(inputs)
        sim.add_probe("mass", "h", reduce="integral")
        sim.add_recorder("crest", "h", every=3, nodes=slice(None, None, 64), pool="max")
        sim.add_statistic("hvar", "h", stat="var", every=3)
        if with_spectra:
            for name, expr, modes, every in specs:
                sim.add_spectrum(name, expr, modes=modes, every=every)
        for _ in range(6):
            next(sim)
        if with_spectra:
            sim.remove_spectrum("b")
            assert list(sim.spectra) == ["a"]
        for _ in range(4):
            next(sim)
        return sim.probes, sim.recorders, sim.statistics, sim.spectra
    p1, r1, s1, c1 = run(True)
    p0, r0, s0, _ = run(False)
    assert np.array_equal(p1["mass"][0], p0["mass"][0]) and p1["mass"][1].tobytes() == p0["mass"][1].tobytes()
    assert np.array_equal(r1["crest"][0], r0["crest"][0]) and r1["crest"][2].tobytes() == r0["crest"][2].tobytes()
    assert s1["hvar"][0] == s0["hvar"][0] == 4 and s1["hvar"][2].tobytes() == s0["hvar"][2].tobytes()
    assert p1["mass"][1].shape == (11,) and r1["crest"][2].shape[0] == 4
    assert_spectra(model_of(inputs[0]), specs[:1], c1, states_of(inputs, 10), inputs[2], label="together")


def test_solver_change_keeps_the_rows():
    """A Python hook hands the run a per-node parameter after step 4 of 8: the next step runs on the solver
    of that parameter layout, and the spectra go on there; no row is lost."""
    inputs = film_inputs(4096)
    name, fields, pars, dt, _ = inputs
    model = model_of(name)
    x = np.asarray(fields["x"])
    specs = specs_of(FILM_EXPRS, 4096)

    def hook(t, f, p):
        if t > 3.5 * dt and np.ndim(p["We"]) == 0:
            f["h"] = np.array(f["h"])            # (a host container again: the step binds a solver for it)
            p = dict(p, We=p["We"] * (1.0 + 0.25 * np.cos(2 * np.pi * x / (x[-1] + x[1]))))
        return f, p

    def run(with_spectra):
        sim = simulation((name, fields, pars, dt, hook))
        if with_spectra:
            for sname, expr, modes, every in specs:
                sim.add_spectrum(sname, expr, modes=modes, every=every)
        keys = ["x", *model._dep_vars]
        states, used = [(sim.t, {k: np.array(sim.fields[k]) for k in keys})], [dict(sim.parameters)]
        for _ in range(8):
            t, f = next(sim)
            if not with_spectra:
                states.append((t, {k: np.array(f[k]) for k in keys}))
                used.append(dict(sim.parameters))
        return sim, states, used
    sim, _, _ = run(True)
    got = sim.spectra
    assert len(sim._spectra._bound) == 2                             # two solvers, one handle each
    _, states, used = run(False)
    assert np.ndim(used[4]["We"]) == 0 and np.ndim(used[5]["We"]) == 1
    assert got["a"][2].shape[0] == 9 and got["b"][2].shape[0] == 3
    assert_spectra(model, specs, got, states, used, label="solver change")


def test_adaptive_steps_record_every_emitted_state():
    inputs = film_inputs(4096)
    name, fields, pars = inputs[:3]
    specs = [("a", "h", cases.low_and_top_modes(4096), 1)]
    sim = Simulation(model_of(name), fields, pars, dt=1e-2)          # the default scheme, time_stepping=True
    sim.add_spectrum("a", "h", modes=specs[0][2])
    keys = ["x", *model_of(name)._dep_vars]
    states = [(sim.t, {k: np.array(sim.fields[k]) for k in keys})]
    sim.add_post_process("keep", lambda s: states.append((s.t, {k: np.array(s.fields[k]) for k in keys})))
    states.pop()                                                     # (add_post_process ran it once)
    for _ in range(6):
        next(sim)
    got = sim.spectra
    assert len(states) == 7 and got["a"][2].shape[0] == 7 and np.all(np.diff(got["a"][0]) > 0)
    assert_spectra(model_of(name), specs, got, states, pars, label="adaptive")
