"""Device histograms on the MI355X: the series against the referee (tests/hist_cases.py) on the same states
-- exactly, every count --, values on the edges, a NaN node, bitwise reproducibility and the ring, residency
of the state and the size of the fetches, ensembles, the six kinds of observers together, a histogram
removed and a change of solver in the middle of a run, adaptive steps."""
import numpy as np
import pytest

from tests import hist_cases as cases
from tests.test_gpu_recorders import _ensemble_case, film_inputs, m1_inputs, model_of, simulation, states_of
from tests.test_statistics import numpy_nodes
from triflow_amd import Simulation
from triflow_amd._capi import DeviceHistogram, DeviceSolver
from triflow_amd.device import DirichletHook
from triflow_amd.ensemble import Ensemble

pytestmark = pytest.mark.gpu

# Expressions the recorders' tests hold bit-equal to NumPy (no non-square integer power of a node value).
# (name, expression, keywords of add_histogram).  The film's h starts as 1 + 0.1 cos: 256 uniform bins over
# (0.85, 1.15) see every step; its capillary term is of either sign and spans decades: explicit edges,
# symmetric and logarithmic.  The advection model's U = cos + x lies in (-1, 2); c * dxU**2 is >= 0.
LOG_EDGES = np.concatenate([-np.logspace(-3, -8, 21), [0.0], np.logspace(-8, -3, 21)])
FILM_HISTS = [("pdf", "h", dict(bins=256, range=(0.85, 1.15))),
              ("cap", "We * h * dxxxh", dict(bins=LOG_EDGES, every=3))]
M1_HISTS = [("u", "U", dict(bins=64, range=(-1.0, 2.0), nodes=slice(1000, 90000, 8))),
            ("g", "c * dxU**2", dict(bins=np.concatenate([[0.0], np.logspace(-4, 2, 25)]), every=3,
                                     nodes=slice(1000, 90000, 8))),
            ("all", "U", dict(bins=[-1.0, 0.0, 0.25, 2.0]))]


def edges_of(kw):
    b = kw["bins"]
    return np.linspace(*kw["range"], b + 1) if isinstance(b, int) else np.asarray(b, dtype=float)


def run_with(inputs, specs, steps, capacity=None, **kw):
    sim = simulation(inputs, **kw)
    for name, expr, k in specs:
        sim.add_histogram(name, expr, capacity=capacity, **k)
    for _ in range(steps):
        next(sim)
    return sim


def assert_histograms(model, specs, got, states, pars, first=None, label=""):
    """``got`` (a front end's ``histograms``) against the referee on ``states = [(t, fields), ...]``; ``pars``:
    the parameters, or one dict per state; ``first``: per histogram, the index of the state of its first row
    (default 0).  Everything is exact: t, the edges, every count of every row."""
    exprs = []
    for _, e, _ in specs:
        if e not in exprs:
            exprs.append(e)
    per_state = pars if isinstance(pars, list) else [pars] * len(states)
    nodes = [numpy_nodes(model, exprs, f, p) for (_, f), p in zip(states, per_state)]
    for name, e, kw in specs:
        idx = list(range((first or {}).get(name, 0), len(states), kw.get("every", 1)))
        t, edges, counts, outside = got[name]
        want = edges_of(kw)
        window = kw.get("nodes", slice(None))
        assert np.array_equal(t, np.array([states[i][0] for i in idx])), name
        assert edges.dtype == np.float64 and edges.tobytes() == want.tobytes(), name
        assert counts.shape == (len(idx), want.size - 1) and counts.dtype == np.int64, (name, counts.shape)
        assert outside.shape == (len(idx), 3) and outside.dtype == np.int64, (name, outside.shape)
        for row, i in enumerate(idx):
            v = nodes[i][exprs.index(e)][window]
            rc, ro = cases.referee(v, want)
            assert np.array_equal(counts[row], rc), (label, name, row, np.flatnonzero(counts[row] != rc))
            assert np.array_equal(outside[row], ro), (label, name, row, outside[row], ro)
            assert counts[row].sum() + outside[row].sum() == v.size, (label, name, row)


@pytest.mark.parametrize("inputs,specs", [(film_inputs(20011), FILM_HISTS), (m1_inputs(100003), M1_HISTS)],
                         ids=["film-ragged-replayed", "M1-clamped-ragged-windowed"])
def test_series_equal_the_referee_on_the_same_states(inputs, specs):
    """Film model at 20 011 nodes: ragged chunks, three workgroups, graph replay on (below 5e4 nodes): the
    row index and the slot are arguments of the launches, a replayed step must not freeze them.  The
    advection model at 100 003 nodes: clamped ends, a window with a step."""
    steps = 12
    got = run_with(inputs, specs, steps).histograms
    states = states_of(inputs, steps)
    assert_histograms(model_of(inputs[0]), specs, got, states, inputs[2], label=inputs[0])
    assert got[specs[0][0]][2].shape[0] == 13 and got[specs[1][0]][2].shape[0] == 5
    if inputs[0] == "M3_film":
        for name, _, _ in specs:
            c = got[name][2]
            assert len({row.tobytes() for row in c}) == c.shape[0], name      # the rows are distinct
            assert (got[name][3] == 0).all() and np.count_nonzero(c[0]) > 8, name


def test_values_on_the_edges_at_t0():
    """An initial h whose nodes cycle through the edges, their neighbours one ulp to either side, NaN, the
    infinities and the zeros: the t0 rows decide every tie (no step is taken)."""
    name, fields, pars, dt, _ = film_inputs(20011)
    for k, (edges, uniform) in enumerate(cases.edge_sets()):
        v = cases.cycled(cases.adversarial(edges), 20011, seed=k)
        sim = simulation((name, dict(fields, h=v), pars, dt, None))
        kw = dict(bins=uniform[0], range=uniform[1:]) if uniform else dict(bins=edges)
        sim.add_histogram("ties", "h", **kw)
        sim.add_histogram("window", "h", nodes=slice(5, -3, 7), **kw)
        for hname, nodes in (("ties", slice(None)), ("window", slice(5, -3, 7))):
            t, e, counts, outside = sim.histograms[hname]
            rc, ro = cases.referee(v[nodes], edges)
            assert e.tobytes() == edges.tobytes() and counts.shape == (1, edges.size - 1)
            assert np.array_equal(counts[0], rc), (k, hname, np.flatnonzero(counts[0] != rc))
            assert np.array_equal(outside[0], ro) and ro[2] > 0 and ro[0] > 0 and ro[1] > 0, (k, hname, outside, ro)
            if uniform:
                cases.check_against_numpy(v[nodes], edges, uniform)


def test_nodes_pinned_to_an_edge_by_a_dirichlet_hook():
    """The hook writes exactly an inner edge into node 0 and exactly edges[-1] into node N - 1 on the device:
    the first belongs to the bin it opens, the second to the last bin, not above."""
    name, fields, pars, dt, _ = m1_inputs(20011)
    edges = np.linspace(-1.0, 2.0, 65)
    inner, top = float(edges[40]), float(edges[-1])
    inputs = (name, fields, pars, dt, DirichletHook(U={0: inner, -1: top}))
    specs = [("u", "U", dict(bins=64, range=(-1.0, 2.0))), ("ends", "U", dict(bins=64, range=(-1.0, 2.0),
                                                                            nodes=slice(0, None, 20010)))]
    steps = 6
    got = run_with(inputs, specs, steps).histograms
    states = states_of(inputs, steps)
    for _, f in states[1:]:
        assert f["U"][0] == inner and f["U"][-1] == top
    assert_histograms(model_of(name), specs, got, states, pars, label="pinned")
    ends = got["ends"][2]
    assert (ends[1:, 40] == 1).all() and (ends[1:, 63] == 1).all() and (ends[1:].sum(1) == 2).all()
    assert (got["ends"][3][1:] == 0).all()


def test_a_row_with_a_nan_node():
    name, fields, pars, dt, _ = film_inputs(4099)
    sim = simulation((name, fields, pars, dt, None))
    sim.fields["h"][1234] = np.nan
    sim.add_histogram("pdf", "h", bins=64, range=(0.0, 3.0))
    sim.add_histogram("elsewhere", "h", bins=64, range=(0.0, 3.0), nodes=slice(0, 1234))
    t, e, counts, outside = sim.histograms["pdf"]
    rc, ro = cases.referee(np.asarray(sim.fields["h"]), e)
    assert np.array_equal(counts[0], rc) and list(outside[0]) == [0, 0, 1] == list(ro)
    assert counts[0].sum() == 4098
    assert list(sim.histograms["elsewhere"][3][0]) == [0, 0, 0] and sim.histograms["elsewhere"][2][0].sum() == 1234


def test_two_runs_are_bit_identical_and_the_ring_wraps():
    inputs = film_inputs(20011)
    small = run_with(inputs, FILM_HISTS, 49, capacity=4).histograms      # 50 and 17 rows through 4
    whole = run_with(inputs, FILM_HISTS, 49).histograms
    again = run_with(inputs, FILM_HISTS, 49).histograms
    for name, _, kw in FILM_HISTS:
        rows = len(range(0, 50, kw.get("every", 1)))
        assert small[name][2].shape[0] == rows and np.array_equal(small[name][0], whole[name][0]), name
        for part in (2, 3):
            assert small[name][part].tobytes() == whole[name][part].tobytes(), name
            assert again[name][part].tobytes() == whole[name][part].tobytes(), name
        assert len({row.tobytes() for row in small[name][2]}) == rows, name       # every row once
        assert (whole[name][2].sum(1) + whole[name][3].sum(1) == 20011).all(), name


def test_state_stays_resident_and_the_fetches_are_rows_of_counts(monkeypatch):
    calls = dict(up=0, down=0, fetch=0, doubles=0)
    for meth, key in (("set_state", "up"), ("get_state", "down"), ("get_state_flat", "down")):
        orig = getattr(DeviceSolver, meth)

        def counted(self, *a, _orig=orig, _key=key, **k):
            calls[_key] += 1
            return _orig(self, *a, **k)
        monkeypatch.setattr(DeviceSolver, meth, counted)
    orig_fetch = DeviceHistogram._fetch

    def fetch(self, ncols, *which):
        out = orig_fetch(self, ncols, *which)
        calls["fetch"] += 1
        calls["doubles"] += out.size
        return out
    monkeypatch.setattr(DeviceHistogram, "_fetch", fetch)
    N = 200_000
    inputs = film_inputs(N)
    sim = simulation(inputs)
    sim.add_histogram("a", "h", bins=64, range=(0.85, 1.15))
    sim.add_histogram("b", "We * h * dxxxh", bins=256, range=(-1e-4, 1e-4), every=3)
    # (the initial state is a host container: every add_histogram before the first step uploads it for its
    # t0 row, as add_probe does; the second add fetched the t0 row of the first.  The run starts here)
    calls.update(up=0, down=0, fetch=0, doubles=0)
    for _ in range(60):
        t, f = next(sim)
        assert f._device_backing() is not None and f._device_backing().valid()
    assert calls == dict(up=1, down=0, fetch=0, doubles=0), calls
    got = sim.histograms
    assert got["a"][2].shape == (61, 64) and got["b"][2].shape == (21, 256)
    assert calls == dict(up=1, down=0, fetch=2, doubles=60 * (64 + 3) + 21 * (256 + 3)), calls
    for name in ("a", "b"):
        assert (got[name][2].sum(1) + got[name][3].sum(1) == N).all(), name


ENSEMBLE_HISTS = [("pdf", "h", dict(bins=256, range=(0.85, 1.15))),
                  ("cap", "We * h * dxxxh", dict(bins=LOG_EDGES, every=3, nodes=slice(1, 4000, 3)))]


def test_ensemble_members():
    """8 members of 4096 nodes with parameters of their own, every member against the referee on the
    ensemble's own states."""
    model, fields, fdict, member_pars, dt = _ensemble_case()
    nsys = 8
    ens = Ensemble(model, fields["x"], fdict, member_pars, periodic=True, scheme="ROS2")
    for name, expr, kw in ENSEMBLE_HISTS:
        ens.add_histogram(name, expr, **kw)
    states = [(ens.t, ens.state())]
    for _ in range(9):
        ens.step(dt)
        states.append((ens.t, ens.state()))
    got = ens.histograms
    ens.close()
    assert got["pdf"][2].shape == (10, nsys, 256) and got["pdf"][3].shape == (10, nsys, 3)
    assert got["cap"][2].shape == (4, nsys, LOG_EDGES.size - 1) and got["cap"][1].shape == (LOG_EDGES.size,)
    assert len({got["cap"][2][:, e].tobytes() for e in range(nsys)}) == nsys     # the members differ
    for e in range(nsys):
        pe = {k: (v[e] if np.ndim(v) else v) for k, v in member_pars.items()}
        mine = [(t, dict(x=fields["x"], **{k: st[j, e] for j, k in enumerate(model._dep_vars)})) for t, st in states]
        assert_histograms(model, ENSEMBLE_HISTS, {k: (t, ed, c[:, e], o[:, e]) for k, (t, ed, c, o) in got.items()},
                          mine, pe, label="member %d" % e)


def test_all_six_observers_together_and_one_removed_mid_run():
    inputs = film_inputs(100003)

    def run(with_histograms):
        sim = simulation(inputs)
        sim.add_probe("mass", "h", reduce="integral")
        sim.add_recorder("crest", "h", every=3, nodes=slice(None, None, 64), pool="max")
        sim.add_statistic("hvar", "h", stat="var", every=3)
        sim.add_spectrum("hk", "h", modes=[1, 4, 8], every=2)
        sim.add_extrema("crests", "h", max_count=8)
        if with_histograms:
            for name, expr, kw in FILM_HISTS:
                sim.add_histogram(name, expr, **kw)
        for _ in range(6):
            next(sim)
        if with_histograms:
            sim.remove_histogram("cap")
            assert list(sim.histograms) == ["pdf"]
        for _ in range(4):
            next(sim)
        return sim.probes, sim.recorders, sim.statistics, sim.spectra, sim.extrema, sim.histograms
    p1, r1, s1, c1, e1, h1 = run(True)
    p0, r0, s0, c0, e0, h0 = run(False)
    assert h0 == {}
    assert np.array_equal(p1["mass"][0], p0["mass"][0]) and p1["mass"][1].tobytes() == p0["mass"][1].tobytes()
    assert np.array_equal(r1["crest"][0], r0["crest"][0]) and r1["crest"][2].tobytes() == r0["crest"][2].tobytes()
    assert s1["hvar"][0] == s0["hvar"][0] == 4 and s1["hvar"][2].tobytes() == s0["hvar"][2].tobytes()
    assert c1["hk"][2].tobytes() == c0["hk"][2].tobytes() and c1["hk"][2].shape == (6, 3)
    for part in range(5):
        assert e1["crests"][part].tobytes() == e0["crests"][part].tobytes(), part
    assert p1["mass"][1].shape == (11,) and r1["crest"][2].shape[0] == 4 and e1["crests"][1].shape == (11,)
    assert_histograms(model_of(inputs[0]), FILM_HISTS[:1], h1, states_of(inputs, 10), inputs[2], label="together")


def test_solver_change_keeps_the_rows():
    """A Python hook hands the run a per-node parameter after step 4 of 8: the next step runs on the solver
    of that parameter layout, and the histograms go on there; no row is lost."""
    inputs = film_inputs(4096)
    name, fields, pars, dt, _ = inputs
    model = model_of(name)
    x = np.asarray(fields["x"])

    def hook(t, f, p):
        if t > 3.5 * dt and np.ndim(p["We"]) == 0:
            f["h"] = np.array(f["h"])            # (a host container again: the step binds a solver for it)
            p = dict(p, We=p["We"] * (1.0 + 0.25 * np.cos(2 * np.pi * x / (x[-1] + x[1]))))
        return f, p

    def run(with_histograms):
        sim = simulation((name, fields, pars, dt, hook))
        if with_histograms:
            for hname, expr, kw in FILM_HISTS:
                sim.add_histogram(hname, expr, **kw)
        keys = ["x", *model._dep_vars]
        states, used = [(sim.t, {k: np.array(sim.fields[k]) for k in keys})], [dict(sim.parameters)]
        for _ in range(8):
            t, f = next(sim)
            if not with_histograms:
                states.append((t, {k: np.array(f[k]) for k in keys}))
                used.append(dict(sim.parameters))
        return sim, states, used
    sim, _, _ = run(True)
    got = sim.histograms
    assert len(sim._histograms._bound) == 2                          # two solvers, one handle each
    _, states, used = run(False)
    assert np.ndim(used[4]["We"]) == 0 and np.ndim(used[5]["We"]) == 1
    assert got["pdf"][2].shape[0] == 9 and got["cap"][2].shape[0] == 3
    assert_histograms(model, FILM_HISTS, got, states, used, label="solver change")


def test_adaptive_steps_record_every_emitted_state():
    inputs = film_inputs(4096)
    name, fields, pars = inputs[:3]
    specs = FILM_HISTS[:1]
    sim = Simulation(model_of(name), fields, pars, dt=1e-2)          # the default scheme, time_stepping=True
    sim.add_histogram("pdf", "h", **specs[0][2])
    keys = ["x", *model_of(name)._dep_vars]
    states = [(sim.t, {k: np.array(sim.fields[k]) for k in keys})]
    sim.add_post_process("keep", lambda s: states.append((s.t, {k: np.array(s.fields[k]) for k in keys})))
    states.pop()                                                     # (add_post_process ran it once)
    for _ in range(6):
        next(sim)
    got = sim.histograms
    assert len(states) == 7 and got["pdf"][2].shape[0] == 7 and np.all(np.diff(got["pdf"][0]) > 0)
    assert_histograms(model_of(name), specs, got, states, pars, label="adaptive")
