"""bench.py's plain run and its --dump-outputs: the writer of the outputs on the host, and
(-m gpu) a plain run end to end, whose outputs are the state an Ensemble reaches in the same
number of steps."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench


class _Model:
    _dep_vars = ("h", "q", "T")


def test_dump_outputs_whole_state(tmp_path):
    bench = _bench()
    state = np.random.default_rng(1).standard_normal((3, 2, 1000))
    bench.dump_outputs(str(tmp_path / "one"), _Model(), state)
    bench.dump_outputs(str(tmp_path / "ranks"), _Model(), state, rank=1, world=2)
    for k, name in enumerate(_Model._dep_vars):
        a = np.load(tmp_path / "one" / (name + ".npy"))
        assert a.dtype == np.float64 and np.array_equal(a, state[k])
        assert np.array_equal(np.load(tmp_path / "ranks" / (name + "_rank1.npy")), state[k])


def test_dump_outputs_sample_is_fixed_and_bounded(tmp_path, monkeypatch):
    """Above the budget: the same seeded nodes for every variable, member and run."""
    bench = _bench()
    monkeypatch.setattr(bench, "DUMP_BYTES", 3 * 2 * 8 * 100)
    state = np.random.default_rng(2).standard_normal((3, 2, 1000))
    for run in ("a", "b"):
        bench.dump_outputs(str(tmp_path / run), _Model(), state)
    out = {run: [np.load(tmp_path / run / (n + ".npy")) for n in _Model._dep_vars] for run in ("a", "b")}
    assert sum(a.nbytes for a in out["a"]) <= bench.DUMP_BYTES
    nodes = [int(np.flatnonzero(state[0, 0] == v)[0]) for v in out["a"][0][0]]
    assert len(set(nodes)) == 100 and nodes == sorted(nodes)
    for k in range(3):
        assert np.array_equal(out["a"][k], out["b"][k])
        assert np.array_equal(out["a"][k], state[k][:, nodes])


@pytest.mark.gpu
def test_plain_run_times_its_steps_and_dumps_them(tmp_path):
    steps, warmup, nodes = 7, 2, 20000
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--nodes", str(nodes),
                          "--steps", str(steps), "--warmup", str(warmup), "--dump-outputs", str(tmp_path)],
                         cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-3000:]
    line = json.loads(res.stdout.strip().splitlines()[-1])
    assert line["steps"] == steps and line["warmup"] == warmup and line["timing"]["repeats"] == 1
    assert line["unit"] == "steps/s" and line["higher_is_better"] is True and line["dtype"] == "f64"
    assert line["ms_per_step"] > 0 and abs(line["value"] * line["ms_per_step"] - 1e3) <= 1e-9 * 1e3
    assert not {"roofline", "kernels_ms_per_step", "scheme_api_steps_per_s", "cpu_baseline", "parity"} & set(line)

    from triflow_amd import Model, workloads
    from triflow_amd.ensemble import Ensemble
    bench = _bench()
    name, x, fields, pars, dt, scheme = bench.build_problem(3, nodes, bench.member_table(1, None))
    model = Model(*workloads.model_args(name))
    ens = Ensemble(model, x, fields, pars, bool(pars["periodic"]), scheme=scheme, nstate=3)
    for _ in range(warmup + steps):
        ens.step(dt)
    ens.sync()
    want = ens.state()
    ens.close()
    assert sorted(os.listdir(tmp_path)) == sorted(n + ".npy" for n in model._dep_vars)
    for k, var in enumerate(model._dep_vars):
        got = np.load(tmp_path / (var + ".npy"))
        assert got.dtype == np.float64 and got.shape == (1, nodes)
        assert np.array_equal(got, want[k]), (var, np.abs(got - want[k]).max())
