"""Device recorders on the MI355X: rows against NumPy on the same states, the ring of two halves,
bitwise reproducibility, residency of the state, adaptive steps, graph replay, ensembles, probes and
recorders together, the container of a recorded series."""
import math

import numpy as np
import pytest
from sympy import lambdify

from oracle import numpy_path as ora
from triflow_amd import Model, Simulation, probes, schemes, workloads
from triflow_amd._capi import DeviceRecord, DeviceSolver
from triflow_amd.container import retrieve_container
from triflow_amd.device import DirichletHook
from triflow_amd.ensemble import Ensemble

pytestmark = pytest.mark.gpu

# (name, expression, keywords of add_recorder): two expressions, every 1 and 3, four geometries.  (No cube
# of a node value: x**3 is lowered to the correctly rounded power, and a NumPy that evaluates it with a
# vectorised pow of its own is an ulp off that at a few nodes in a hundred -- DESIGN.md section 15.)
FILM_RECS = [("h_xt", "h", dict(every=1, nodes=slice(None, None, 64))),
             ("crest", "h", dict(every=3, nodes=slice(None, None, 64), pool="max")),
             ("trough", "h", dict(every=1, nodes=slice(2000, 6000, 8), pool="min")),
             ("flux", "We * h * dxxxh", dict(every=3, nodes=slice(2001, 60000, 100), pool="mean"))]
M1_RECS = [("u", "U", dict(every=1, nodes=slice(None, None, 16))),
           ("low", "U", dict(every=3, nodes=slice(5, None, 50), pool="min")),
           ("grad", "c * dxU**2", dict(every=3, nodes=slice(3, 20000, 7), pool="max")),
           ("gmean", "c * dxU**2", dict(every=1, nodes=slice(None, None, 300), pool="mean"))]

_MODELS = {}


def model_of(name):
    if name not in _MODELS:
        _MODELS[name] = Model(*workloads.model_args(name))
    return _MODELS[name]


def film_inputs(N):
    _, fields, pars, dt, _ = workloads.config_inputs(3, N)
    return "M3_film", fields, pars, dt, None


def m1_inputs(N):
    x = np.linspace(0, 1, N)
    return ("M1_advdiff", dict(x=x, U=np.cos(2 * np.pi * x * 5) + x), dict(c=.03, k=.001, periodic=False), 1e-3,
            DirichletHook(U={0: 1.0, -1: 0.0}))


def bins(values, nodes):
    start, stop, step = nodes.indices(values.size)
    return [values[g:min(g + step, stop)] for g in range(start, stop, step)]


def reference_rows(model, recs, fields, pars):
    """The columns of one downloaded state, in NumPy: the lambdified discretised expressions with the
    reference's module dictionary on the ghost-padded views, then the pools; per recorder
    (columns, bound): bound 0 but for "mean", 2**-52 * fsum(|bin|) there (tests/test_recorders.py)."""
    disc = [probes.discretise(model, r[1]) for r in recs]
    func = lambdify(model._symbolic_args, disc, modules=ora._lambdify_modules())
    inputs = [np.asarray(fields["x"])] + [np.asarray(fields[k]) for k in model._dep_vars] + \
        [pars[k] for k in model._pars] + [pars["periodic"]]
    env, N, _, _ = ora.stencil_views(model, *inputs)
    vals = func(*[env[k] for k in model._args])
    out = []
    for (_, _, kw), v in zip(recs, vals):
        f = np.broadcast_to(np.asarray(v, dtype=float), (N,))
        nodes, pool = kw.get("nodes", slice(None)), kw.get("pool", "sample")
        if pool == "sample":
            out.append((f[nodes], None))
        elif pool in ("max", "min"):
            out.append((np.array([getattr(np, pool)(b) for b in bins(f, nodes)]), None))
        else:
            out.append((np.array([math.fsum(b) / b.size for b in bins(f, nodes)]),
                        np.array([2.0 ** -52 * math.fsum(np.abs(b)) for b in bins(f, nodes)])))
    return out


def assert_row(name, got, ref, bound):
    assert got.shape == ref.shape, name
    if bound is None:
        assert np.array_equal(got, ref), (name, np.abs(got - ref).max())
    else:
        err = np.abs(got - ref)
        print(name, "mean: worst error / bound %.3g" % np.max(err / np.maximum(bound, 1e-300)))
        assert (err <= bound).all(), (name, np.max(err / np.maximum(bound, 1e-300)))


def simulation(inputs, scheme=schemes.ROS2, **kw):
    name, fields, pars, dt, hook = inputs
    kw.setdefault("time_stepping", False)
    if hook is not None:
        kw["hook"] = hook
    return Simulation(model_of(name), fields, pars, dt=dt, scheme=scheme, **kw)


def recorded_run(inputs, recs, steps, capacity=None):
    sim = simulation(inputs)
    for rname, expr, kw in recs:
        sim.add_recorder(rname, expr, capacity=capacity, **kw)
    for _ in range(steps):
        next(sim)
    return sim.recorders


def states_of(inputs, steps, **kw):
    """The same run again, its state downloaded after every step (the steps are bitwise deterministic)."""
    model = model_of(inputs[0])
    sim = simulation(inputs, **kw)
    keys = ["x", *model._dep_vars]
    states = [(sim.t, {k: np.array(sim.fields[k]) for k in keys})]
    for _ in range(steps):
        t, f = next(sim)
        states.append((t, {k: np.array(f[k]) for k in keys}))
    return states


@pytest.mark.parametrize("inputs", [film_inputs(10 ** 6), film_inputs(100003), m1_inputs(20011)],
                         ids=["film-1e6", "film-ragged", "M1-clamped-ragged"])
def test_rows_match_numpy_on_the_same_states(inputs):
    name, pars = inputs[0], inputs[2]
    recs = FILM_RECS if name == "M3_film" else M1_RECS
    steps = 12
    got = recorded_run(inputs, recs, steps)
    states = states_of(inputs, steps)
    model = model_of(name)
    x = np.asarray(inputs[1]["x"])
    for rname, _, kw in recs:
        t, xr, values = got[rname]
        due = list(range(0, steps + 1, kw["every"]))
        assert np.array_equal(t, np.array([states[i][0] for i in due])), rname
        assert np.array_equal(xr, x[kw["nodes"]]) and values.shape == (len(due), xr.size), rname
    for i, (t, state) in enumerate(states):
        ref = reference_rows(model, recs, state, pars)
        for (rname, _, kw), (cols, bound) in zip(recs, ref):
            if i % kw["every"] == 0:
                assert_row((rname, i), got[rname][2][i // kw["every"]], cols, bound)
    sample = got[recs[0][0]][2]
    assert not np.array_equal(sample[0], sample[1]) and not np.array_equal(sample[-2], sample[-1])


def test_ring_wraps_and_two_runs_are_bit_identical():
    inputs = film_inputs(100003)
    small = recorded_run(inputs, FILM_RECS, 49, capacity=4)       # h_xt, trough: 50 rows through 4
    whole = recorded_run(inputs, FILM_RECS, 49)
    again = recorded_run(inputs, FILM_RECS, 49)
    for rname, _, kw in FILM_RECS:
        rows = len(range(0, 50, kw["every"]))
        assert small[rname][2].shape[0] == rows and np.array_equal(small[rname][0], whole[rname][0])
        assert np.all(np.diff(small[rname][0]) > 0)
        assert small[rname][2].tobytes() == whole[rname][2].tobytes(), rname
        assert again[rname][2].tobytes() == whole[rname][2].tobytes(), rname
        assert len({row.tobytes() for row in small[rname][2]}) == rows, rname        # every row once


def test_state_stays_resident(monkeypatch):
    calls = dict(up=0, down=0, fetch=0, rows=0)
    for meth, key in (("set_state", "up"), ("get_state", "down"), ("get_state_flat", "down")):
        orig = getattr(DeviceSolver, meth)

        def counted(self, *a, _orig=orig, _key=key, **k):
            calls[_key] += 1
            return _orig(self, *a, **k)
        monkeypatch.setattr(DeviceSolver, meth, counted)
    orig_fetch = DeviceRecord.fetch

    def fetch(self, which):
        out = orig_fetch(self, which)
        calls["fetch"] += 1
        calls["rows"] += out.size
        return out
    monkeypatch.setattr(DeviceRecord, "fetch", fetch)
    inputs = film_inputs(200_000)
    sim = simulation(inputs)
    for rname, expr, kw in FILM_RECS[:2]:
        sim.add_recorder(rname, expr, capacity=16, **kw)
    # (the initial state is a host container: every add_recorder before the first step uploads it for its
    # t0 row, as add_probe does; the run itself starts here)
    calls.update(up=0, down=0)
    for _ in range(60):
        t, f = next(sim)
        assert f._device_backing() is not None and f._device_backing().valid()
    assert calls["up"] == 1 and calls["down"] == 0, calls
    series = sim.recorders
    assert calls["up"] == 1 and calls["down"] == 0, calls
    ncols = 200_000 // 64
    assert series["h_xt"][2].shape == (61, ncols) and series["crest"][2].shape == (21, ncols)
    assert calls["rows"] <= 82 * ncols, calls              # rows only (the t0 rows were fetched at the second add)


def test_adaptive_steps_record_every_accepted_step():
    inputs = film_inputs(4096)
    name, fields, pars = inputs[:3]
    recs = FILM_RECS[:1] + [("crest8", "h", dict(every=1, nodes=slice(None, None, 8), pool="max"))]
    sim = Simulation(model_of(name), fields, pars, dt=1e-2)          # the default scheme, time_stepping=True
    for rname, expr, kw in recs:
        sim.add_recorder(rname, expr, **kw)
    keys = ["x", *model_of(name)._dep_vars]
    states = [(sim.t, {k: np.array(sim.fields[k]) for k in keys})]
    sim.add_post_process("keep", lambda s: states.append((s.t, {k: np.array(s.fields[k]) for k in keys})))
    states.pop()                                                     # (add_post_process ran it once)
    for _ in range(6):
        next(sim)
    got = sim.recorders
    assert len(states) == 7
    for rname, _, _ in recs:
        assert np.array_equal(got[rname][0], np.array([s[0] for s in states]))
        assert np.all(np.diff(got[rname][0]) > 0)
    for i, (t, state) in enumerate(states):
        for (rname, _, _), (cols, bound) in zip(recs, reference_rows(model_of(name), recs, state, pars)):
            assert_row((rname, i), got[rname][2][i], cols, bound)


def test_small_grid_with_graph_replay():
    """Config 3 at 20 000 nodes (graph replay on by default below 5e4 nodes): a replayed step must not
    freeze the row or the slot (the record launches are outside the captured step)."""
    inputs = film_inputs(20_000)
    steps = 30
    got = recorded_run(inputs, FILM_RECS[:3], steps)
    states = states_of(inputs, steps)
    h = got["h_xt"][2]
    assert h.shape[0] == steps + 1
    assert all(not np.array_equal(h[i], h[i + 1]) for i in range(steps))
    for i, (t, state) in enumerate(states):
        ref = reference_rows(model_of(inputs[0]), FILM_RECS[:3], state, inputs[2])
        for (rname, _, kw), (cols, bound) in zip(FILM_RECS[:3], ref):
            if i % kw["every"] == 0:
                assert_row((rname, i), got[rname][2][i // kw["every"]], cols, bound)


def _ensemble_case():
    name, fields, pars, dt, _ = film_inputs(4096)
    model = model_of(name)
    member_pars = dict(pars)
    member_pars["We"] = np.array([.01, .02, .005, .015, .012, .018, .008, .011])
    member_pars["c"] = np.array([1., .5, 1.5, .8, 1.1, .9, 1.3, .7])
    fdict = {k: np.tile(fields[k], (8, 1)) for k in model._dep_vars}
    return model, fields, fdict, member_pars, dt


ENSEMBLE_RECS = FILM_RECS[:2] + [("flux", "We * h * dxxxh", dict(every=3, nodes=slice(1, 4000, 100), pool="mean"))]


def test_ensemble_rows_match_numpy_on_the_members_states():
    model, fields, fdict, member_pars, dt = _ensemble_case()
    nsys = 8
    ens = Ensemble(model, fields["x"], fdict, member_pars, periodic=True, scheme="ROS2")
    for rname, expr, kw in ENSEMBLE_RECS:
        ens.add_recorder(rname, expr, **kw)
    states = [ens.state()]
    for _ in range(9):
        ens.step(dt)
        states.append(ens.state())
    got = ens.recorders
    ens.close()
    assert got["h_xt"][2].shape == (10, nsys, 64) and got["crest"][2].shape == (4, nsys, 64)
    assert got["h_xt"][1].shape == (64,) and np.allclose(got["flux"][0], [0, 3 * dt, 6 * dt, 9 * dt])
    for e in range(nsys):
        pe = {k: (v[e] if np.ndim(v) else v) for k, v in member_pars.items()}
        for i, st in enumerate(states):
            f = dict(x=fields["x"], **{k: st[j, e] for j, k in enumerate(model._dep_vars)})
            for (rname, _, kw), (cols, bound) in zip(ENSEMBLE_RECS, reference_rows(model, ENSEMBLE_RECS, f, pe)):
                if i % kw["every"] == 0:
                    assert_row((rname, e, i), got[rname][2][i // kw["every"], e], cols, bound)


def test_ensemble_members_equal_single_runs():
    """Member e's rows of h (sampled, and the maximum of every bin) are the rows of a single-system run of
    member e, bit for bit.  The comparison stops at the state variables: the states of an 8-member and of
    a 1-member solver differ in the last bits (measured here: up to 5.6e-16 after 9 steps, the solver's
    partition depends on the number of systems), and an expression like We*h*dxxxh, which divides
    differences of h by dx**3, shows that as different rows -- its rows are checked against NumPy on the
    ensemble's own states above."""
    model, fields, fdict, member_pars, dt = _ensemble_case()
    recs = ENSEMBLE_RECS[:2]

    def run(fd, p):
        ens = Ensemble(model, fields["x"], fd, p, periodic=True, scheme="ROS2")
        for rname, expr, kw in recs:
            ens.add_recorder(rname, expr, **kw)
        for _ in range(9):
            ens.step(dt)
        out = ens.recorders
        ens.close()
        return out
    got = run(fdict, member_pars)
    for e in range(8):
        pe = {k: (v[e] if np.ndim(v) else v) for k, v in member_pars.items()}
        one = run({k: v[e:e + 1] for k, v in fdict.items()}, pe)
        for rname, _, _ in recs:
            assert np.array_equal(one[rname][0], got[rname][0])
            assert one[rname][2][:, 0].tobytes() == got[rname][2][:, e].tobytes(), (rname, e)


def test_probes_and_recorders_together():
    inputs = film_inputs(100003)
    plist = [("mass", "h", "integral"), ("crest", "h", "max")]

    def run(with_probes, with_recorders):
        sim = simulation(inputs)
        if with_probes:
            for pname, expr, kind in plist:
                sim.add_probe(pname, expr, reduce=kind)
        if with_recorders:
            for rname, expr, kw in FILM_RECS:
                sim.add_recorder(rname, expr, **kw)
        for _ in range(10):
            next(sim)
        return sim.probes, sim.recorders
    both_p, both_r = run(True, True)
    only_p, _ = run(True, False)
    _, only_r = run(False, True)
    for pname, _, _ in plist:
        assert np.array_equal(both_p[pname][0], only_p[pname][0])
        assert both_p[pname][1].tobytes() == only_p[pname][1].tobytes()
    for rname, _, _ in FILM_RECS:
        assert np.array_equal(both_r[rname][0], only_r[rname][0])
        assert both_r[rname][2].tobytes() == only_r[rname][2].tobytes()


def test_recorder_added_and_removed_mid_run(tmp_path):
    inputs = film_inputs(4096)
    sim = simulation(inputs)
    sim.add_recorder(*FILM_RECS[0][:2], **FILM_RECS[0][2])
    for _ in range(4):
        next(sim)
    t_added = sim.t
    sim.add_recorder("late", "h", every=2, nodes=slice(None, None, 64))
    for _ in range(6):
        next(sim)
    first, late = sim.recorders["h_xt"], sim.recorders["late"]
    assert first[0].shape == (11,) and late[0].shape == (4,) and late[0][0] == t_added
    assert np.array_equal(late[0], first[0][4::2]) and late[2].tobytes() == first[2][4::2].tobytes()
    sim.remove_recorder("late")
    next(sim)
    assert list(sim.recorders) == ["h_xt"] and sim.recorders["h_xt"][2].shape == (12, 64)
    # the container of a device-recorded series
    path = sim.save_recorder("h_xt", str(tmp_path / "h_xt"))
    back = retrieve_container(path)
    t, x, values = sim.recorders["h_xt"]
    assert np.array_equal(back.data["t"], t) and np.array_equal(back.data["x"], x)
    assert np.array_equal(back.data["h_xt"], values)
    assert back.metadata["We"] == inputs[2]["We"] and back.metadata["periodic"] == inputs[2]["periodic"]
