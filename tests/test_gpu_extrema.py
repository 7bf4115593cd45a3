"""Device extrema on the MI355X: the series against the NumPy referee on the same states -- n, g and the
values exactly --, a crafted state with thousands of extrema, overflow of max_count, graph replay, bitwise
reproducibility and the ring, residency of the state, ensembles, the five kinds of observers together, an
observer removed in the middle of a run, adaptive steps."""
import numpy as np
import pytest

from tests import extrema_cases as cases
from tests.test_gpu_recorders import film_inputs, m1_inputs, model_of, simulation, states_of
from tests.test_statistics import numpy_nodes
from triflow_amd import Simulation
from triflow_amd._capi import DeviceExtrema, DeviceSolver
from triflow_amd.ensemble import Ensemble

pytestmark = pytest.mark.gpu

# (name, expression, keywords of add_extrema).  Expressions without non-square integer powers of node values:
# for those NumPy's bits are the device's.
FILM_SPECS = [("crests", "h", dict()),
              ("troughs", "h", dict(kind="min", every=3, refine=False, max_count=64)),
              ("tall", "h", dict(threshold=1.05, max_count=8)),
              ("flux", "We * h * dxxxh", dict(every=3, max_count=1024))]
M1_SPECS = [("u", "U", dict()),
            ("low", "U", dict(kind="min", threshold=0.5, every=3, max_count=3)),
            ("grad", "c * dxU**2", dict(every=3, refine=False)),
            ("gmin", "c * dxU**2", dict(kind="min", max_count=1024))]


def run_with(inputs, specs, steps, capacity=None, **kw):
    sim = simulation(inputs, **kw)
    for name, expr, k in specs:
        sim.add_extrema(name, expr, capacity=capacity, **k)
    for _ in range(steps):
        next(sim)
    return sim


def assert_series(model, specs, got, states, pars, periodic, first=None, label=""):
    """``got`` (a front end's ``extrema``) against the referee on ``states = [(t, fields), ...]``; ``first``:
    per observer, the index of the state of its first row (default 0).  Everything is exact.  Returns the
    largest n met per observer."""
    exprs = []
    for _, e, _ in specs:
        if e not in exprs:
            exprs.append(e)
    nodes = [numpy_nodes(model, exprs, f, pars) for _, f in states]
    x = np.asarray(states[0][1]["x"])
    most = {}
    for name, e, kw in specs:
        idx = list(range((first or {}).get(name, 0), len(states), kw.get("every", 1)))
        t, n, g, xs, vs = got[name]
        mc = kw.get("max_count", 256)
        assert np.array_equal(t, np.array([states[i][0] for i in idx])), name
        assert n.shape == (len(idx),) and n.dtype == np.int64 and g.shape == (len(idx), mc), (name, n.shape, g.shape)
        for row, i in enumerate(idx):
            cases.assert_row((n[row], g[row], xs[row], vs[row]), nodes[i][exprs.index(e)], x, kw.get("kind", "max"),
                             periodic, kw.get("threshold"), mc, kw.get("refine", True), label=(label, name, row))
        most[name] = int(n.max())
        print("%s %s: %d rows, n = %d ... %d" % (label, name, len(idx), n.min(), n.max()))
    return most


@pytest.mark.parametrize("inputs,specs", [(film_inputs(20011), FILM_SPECS), (m1_inputs(100003), M1_SPECS)],
                         ids=["film-ragged-replayed", "M1-clamped-ragged"])
def test_series_match_the_referee_on_the_same_states(inputs, specs):
    steps = 12
    sim = run_with(inputs, specs, steps)
    got = sim.extrema
    most = assert_series(model_of(inputs[0]), specs, got, states_of(inputs, steps), inputs[2],
                         inputs[2]["periodic"], label=inputs[0])
    assert got[specs[0][0]][1].shape == (13,) and got[specs[1][0]][1].shape == (5,)
    assert most[specs[0][0]] >= 1                       # (the waves of the initial state)


def _rough(N, seed=11):
    """Config 3 at N nodes, its film thickness a seeded random perturbation: about a third of the nodes are
    crests."""
    name, fields, pars, dt, hook = film_inputs(N)
    fields = dict(fields, h=1.0 + 1e-3 * np.random.RandomState(seed).standard_normal(N))
    return name, fields, pars, dt, hook


def test_thousands_of_extrema_in_the_row_of_a_crafted_state_and_overflow():
    """The t0 row of a rough state: every chunk border and several workgroups of the scan are crossed.  Then
    max_count=16: the kept prefix is the first 16 of the full row, n is unchanged."""
    N = 20011
    inputs = _rough(N)
    h = inputs[1]["h"]
    rg, rt = cases.referee(h, "max", True)
    assert N // 4 < rg.size < 8192                      # (checked here, on the CPU: the row holds them all)
    sim = simulation(inputs)
    sim.add_extrema("all", "h", max_count=8192, refine=False)
    sim.add_extrema("few", "h", max_count=16, refine=False)
    sim.add_extrema("troughs", "h", kind="min", max_count=8192)
    sim.add_extrema("flux", "We * h * dxxxh", max_count=8192)
    got = sim.extrema
    t, n, g, x, v = got["all"]
    assert n.shape == (1,) and n[0] == rg.size and np.array_equal(g[0, :rg.size], rg) and (g[0, rg.size:] == -1).all()
    assert v[0, :rg.size].tobytes() == rt[:, 1].tobytes() and np.isnan(v[0, rg.size:]).all()
    t, n16, g16, x16, v16 = got["few"]
    assert n16[0] == rg.size and g16.shape == (1, 16)
    assert np.array_equal(g16[0], g[0, :16]) and v16.tobytes() == v[:, :16].tobytes() and x16.tobytes() == x[:, :16].tobytes()
    specs = [("all", "h", dict(max_count=8192, refine=False)), ("few", "h", dict(max_count=16, refine=False)),
             ("troughs", "h", dict(kind="min", max_count=8192)), ("flux", "We * h * dxxxh", dict(max_count=8192))]
    keys = ["x", *model_of(inputs[0])._dep_vars]
    state = [(sim.t, {k: np.asarray(inputs[1][k]) for k in keys})]
    most = assert_series(model_of(inputs[0]), specs, got, state, inputs[2], True, label="rough")
    assert most["flux"] > N // 5


def test_small_grid_with_graph_replay():
    """Config 3 at 20 000 nodes (graph replay on by default below 5e4 nodes): the row index is an argument
    of the launch, and a replayed step must not freeze it or the slot."""
    inputs = film_inputs(20_000)
    steps = 30
    specs = [("crests", "h", dict(max_count=16))]
    got = run_with(inputs, specs, steps).extrema
    assert_series(model_of(inputs[0]), specs, got, states_of(inputs, steps), inputs[2], True, label="replay")
    t, n, g, x, v = got["crests"]
    assert n.shape == (steps + 1,) and len({row.tobytes() for row in v}) == steps + 1


def test_two_runs_are_bit_identical_and_the_ring_wraps():
    inputs = film_inputs(20011)
    specs = FILM_SPECS
    small = run_with(inputs, specs, 49, capacity=4).extrema          # 50 and 17 rows through 4
    whole = run_with(inputs, specs, 49).extrema
    again = run_with(inputs, specs, 49).extrema
    for name, _, kw in specs:
        rows = len(range(0, 50, kw.get("every", 1)))
        assert small[name][1].shape == (rows,) and np.array_equal(small[name][0], whole[name][0]), name
        for j in range(1, 5):
            assert small[name][j].tobytes() == whole[name][j].tobytes(), (name, j)
            assert again[name][j].tobytes() == whole[name][j].tobytes(), (name, j)
    assert len({row.tobytes() for row in small["crests"][4]}) == 50               # every row once


def test_state_stays_resident(monkeypatch):
    calls = dict(up=0, down=0, fetch=0, doubles=0)
    for meth, key in (("set_state", "up"), ("get_state", "down"), ("get_state_flat", "down")):
        orig = getattr(DeviceSolver, meth)

        def counted(self, *a, _orig=orig, _key=key, **k):
            calls[_key] += 1
            return _orig(self, *a, **k)
        monkeypatch.setattr(DeviceSolver, meth, counted)
    orig_fetch = DeviceExtrema._fetch

    def fetch(self, ncols, *which):
        out = orig_fetch(self, ncols, *which)
        calls["fetch"] += 1
        calls["doubles"] += out.size
        return out
    monkeypatch.setattr(DeviceExtrema, "_fetch", fetch)
    inputs = film_inputs(200_000)
    sim = simulation(inputs)
    sim.add_extrema("crests", "h", max_count=8)
    sim.add_extrema("flux", "We * h * dxxxh", kind="min", every=3, max_count=4)
    # (the initial state is a host container: every add_extrema before the first step uploads it for its t0
    # row, as add_probe does; the second add fetched the t0 row of the first.  The run starts here)
    calls.update(up=0, down=0, fetch=0, doubles=0)
    for _ in range(30):
        t, f = next(sim)
        assert f._device_backing() is not None and f._device_backing().valid()
    assert calls == dict(up=1, down=0, fetch=0, doubles=0), calls
    got = sim.extrema
    assert got["crests"][2].shape == (31, 8) and got["flux"][2].shape == (11, 4)
    assert calls == dict(up=1, down=0, fetch=2, doubles=30 * 33 + 11 * 17), calls


def _members(N, hs):
    """An ensemble of config 3 at N nodes, one member per row of ``hs`` (its film thickness), each with
    parameters of its own."""
    name, fields, pars, dt, _ = film_inputs(N)
    model = model_of(name)
    nsys = len(hs)
    member_pars = dict(pars)
    member_pars["We"] = np.array([.01, .02, .005, .015][:nsys])
    member_pars["c"] = np.array([1., .5, 1.5, .8][:nsys])
    fdict = {k: np.tile(fields[k], (nsys, 1)) for k in model._dep_vars}
    fdict["h"] = np.array(hs)
    fdict["q"] = fdict["h"] ** 3
    return model, fields, fdict, member_pars, dt


ENSEMBLE_SPECS = [("crests", "h", dict(max_count=32)),
                  ("flux", "We * h * dxxxh", dict(kind="min", every=3, max_count=512))]


def _assert_members(model, x, specs, got, states, member_pars, label):
    nsys = states[0][1].shape[1]
    counts = []
    for e in range(nsys):
        pe = {k: (v[e] if np.ndim(v) else v) for k, v in member_pars.items()}
        mine = [(t, dict(x=x, **{k: st[j, e] for j, k in enumerate(model._dep_vars)})) for t, st in states]
        most = assert_series(model, specs, {k: (s[0],) + tuple(a[:, e] for a in s[1:]) for k, s in got.items()},
                             mine, pe, True, label="%s member %d" % (label, e))
        counts.append(most[specs[0][0]])
    return counts


def test_ensemble_members_against_the_referee_on_their_own_states():
    """Three members with waves, parameters and so counts of their own: the scan restarts per system."""
    N = 4099
    x = np.linspace(0, 100, N, endpoint=False)
    hs = [1 + 0.1 * np.cos(2 * np.pi * waves * x / 100) for waves in (4, 7, 9)]      # (no crest midway between nodes)
    model, fields, fdict, member_pars, dt = _members(N, hs)
    ens = Ensemble(model, fields["x"], fdict, member_pars, periodic=True, scheme="ROS2")
    for name, expr, kw in ENSEMBLE_SPECS:
        ens.add_extrema(name, expr, **kw)
    states = [(ens.t, ens.state())]
    for _ in range(6):
        ens.step(dt)
        states.append((ens.t, ens.state()))
    got = ens.extrema
    ens.close()
    assert got["crests"][1].shape == (7, 3) and got["crests"][2].shape == (7, 3, 32)
    assert got["flux"][1].shape == (3, 3) and got["flux"][4].shape == (3, 3, 512)
    counts = _assert_members(model, fields["x"], ENSEMBLE_SPECS, got, states, member_pars, "waves")
    assert counts == [4, 7, 9]


def test_ensemble_of_rough_members_at_t0():
    """Three rough members (about N / 3 crests each, different in every member) at their t0 row."""
    N = 4099
    hs = [1.0 + 1e-3 * np.random.RandomState(20 + e).standard_normal(N) for e in range(3)]
    model, fields, fdict, member_pars, dt = _members(N, hs)
    specs = [("crests", "h", dict(max_count=2048)), ("few", "h", dict(kind="min", max_count=5, refine=False))]
    ens = Ensemble(model, fields["x"], fdict, member_pars, periodic=True, scheme="ROS2")
    for name, expr, kw in specs:
        ens.add_extrema(name, expr, **kw)
    states = [(ens.t, ens.state())]
    got = ens.extrema
    ens.close()
    counts = _assert_members(model, fields["x"], specs, got, states, member_pars, "rough")
    assert len(set(counts)) == 3 and min(counts) > N // 4 and max(counts) < 2048


def test_all_five_observers_together_and_one_removed_mid_run():
    inputs = film_inputs(100003)
    specs = [("crests", "h", dict(max_count=8)), ("flux", "We * h * dxxxh", dict(every=2, max_count=64))]

    def run(with_extrema):
        sim = simulation(inputs)
        sim.add_probe("mass", "h", reduce="integral")
        sim.add_recorder("crest", "h", every=3, nodes=slice(None, None, 64), pool="max")
        sim.add_statistic("hvar", "h", stat="var", every=3)
        sim.add_spectrum("hk", "h", modes=[1, 4, 8], every=2)
        if with_extrema:
            for name, expr, kw in specs:
                sim.add_extrema(name, expr, **kw)
        for _ in range(6):
            next(sim)
        if with_extrema:
            sim.remove_extrema("flux")
            assert list(sim.extrema) == ["crests"]
        for _ in range(4):
            next(sim)
        return sim.probes, sim.recorders, sim.statistics, sim.spectra, sim.extrema
    p1, r1, s1, c1, e1 = run(True)
    p0, r0, s0, c0, _ = run(False)
    assert np.array_equal(p1["mass"][0], p0["mass"][0]) and p1["mass"][1].tobytes() == p0["mass"][1].tobytes()
    assert np.array_equal(r1["crest"][0], r0["crest"][0]) and r1["crest"][2].tobytes() == r0["crest"][2].tobytes()
    assert s1["hvar"][0] == s0["hvar"][0] == 4 and s1["hvar"][2].tobytes() == s0["hvar"][2].tobytes()
    assert c1["hk"][2].tobytes() == c0["hk"][2].tobytes() and c1["hk"][2].shape == (6, 3)
    assert p1["mass"][1].shape == (11,) and r1["crest"][2].shape[0] == 4
    assert_series(model_of(inputs[0]), specs[:1], e1, states_of(inputs, 10), inputs[2], True, label="together")


def test_adaptive_steps_record_every_accepted_step():
    inputs = film_inputs(4096)
    name, fields, pars = inputs[:3]
    specs = [("crests", "h", dict(max_count=8)), ("troughs", "h", dict(kind="min", max_count=8, refine=False))]
    sim = Simulation(model_of(name), fields, pars, dt=1e-2)          # the default scheme, time_stepping=True
    for sname, expr, kw in specs:
        sim.add_extrema(sname, expr, **kw)
    keys = ["x", *model_of(name)._dep_vars]
    states = [(sim.t, {k: np.array(sim.fields[k]) for k in keys})]
    sim.add_post_process("keep", lambda s: states.append((s.t, {k: np.array(s.fields[k]) for k in keys})))
    states.pop()                                                     # (add_post_process ran it once)
    for _ in range(6):
        next(sim)
    got = sim.extrema
    assert len(states) == 7 and got["crests"][1].shape == (7,) and np.all(np.diff(got["crests"][0]) > 0)
    assert_series(model_of(name), specs, got, states, pars, True, label="adaptive")
