"""The cost of the exact Heaviside mode in the hottest kernel: viscous Burgers with
``upwind(U, U, 2)`` at N = 1e6,
  sweep_ms    mean duration of the F+J sweep (``tf_eval_repeat``, two HIP events round ``--reps`` sweeps)
  steps_per_s ROS2, fixed dt, through the scheme's device path
in the default mode (``one``: Heaviside == 1) and in ``exact`` mode.  The legs are alternated in one process,
``--rounds`` times; min / median / max per leg and exact over one.  One JSON line per measurement on stdout.

    python tools/gpu_heaviside_rate.py [--N 1000000] [--reps 200] [--steps 200] [--rounds 5] [--modes one,exact]

``--modes one`` builds the model without the keyword: the same script measures a commit from before it.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np  # noqa: E402

from triflow_amd import Model, schemes  # noqa: E402

EQUATION = ("k*dxxU - upwind(U, U, 2)", "U", ["k"])
MODELS = {}


def model_of(mode):
    if mode not in MODELS:
        MODELS[mode] = Model(*EQUATION) if mode == "one" else Model(*EQUATION, heaviside=mode)
    return MODELS[mode]


def inputs(N):
    x = np.linspace(0.0, 1.0, N, endpoint=False)
    return dict(x=x, U=np.sin(2 * np.pi * x) + 0.2), dict(k=1e-3, periodic=True), 1e-7


def sweep_ms(N, mode, reps):
    m = model_of(mode)
    fields, pars, _ = inputs(N)
    cm = m._device
    s = cm.solver(N, True, 1, 0)
    cm.bind_inputs(s, fields["x"], [pars["k"]], None)
    s.set_state(0, np.array([fields["U"]]))
    s.eval_repeat(0, True, 10)
    return s.eval_repeat(0, True, reps)


def steps_per_s(N, mode, steps):
    m = model_of(mode)
    fields, pars, dt = inputs(N)
    scheme = schemes.ROS2(m)
    t, f = 0.0, m.fields_template(**fields)
    for _ in range(5):
        t, f = scheme(t, f, dt, pars)
    np.asarray(f["U"])[0]                           # waits for the queued steps
    t0 = time.perf_counter()
    for _ in range(steps):
        t, f = scheme(t, f, dt, pars)
    np.asarray(f["U"])[0]
    return steps / (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=10 ** 6)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--modes", default="one,exact")
    args = ap.parse_args()
    modes = args.modes.split(",")
    out = {what: {mode: [] for mode in modes} for what in ("sweep_ms", "steps_per_s")}
    for r in range(args.rounds):
        for what, fn, n in (("sweep_ms", sweep_ms, args.reps), ("steps_per_s", steps_per_s, args.steps)):
            for mode in modes:
                v = fn(args.N, mode, n)
                out[what][mode].append(v)
                print(json.dumps(dict(what=what, mode=mode, round=r, N=args.N, value=round(v, 5))), flush=True)
    summary = dict(what="summary", N=args.N)
    for what, legs in out.items():
        summary[what] = {mode: dict(min=round(min(v), 5), median=round(float(np.median(v)), 5), max=round(max(v), 5))
                         for mode, v in legs.items()}
        if "one" in legs and "exact" in legs:
            summary[what + "_exact_over_one"] = round(float(np.median(legs["exact"]) / np.median(legs["one"])), 4)
    print(json.dumps(summary), flush=True)


if __name__ == "__main__":
    main()
