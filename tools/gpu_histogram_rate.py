"""Device histograms at config 3 (film model, N = 1e6, ROS2, fixed dt, Simulation loop): steps/s
  none        no observer (control)
  hist1       64 bins of h over (0.85, 1.15), a row per step
  hist10      the same, a row every 10th step
  cap256      256 bins of We * h * dxxxh over (-1e-4, 1e-4), a row per step
  python1     the post-process ``np.histogram(np.asarray(simul.fields["h"]), 64, (0.85, 1.15))`` after every
              step
The legs are alternated in one process, ``--rounds`` times, blocks of ``--steps`` steps; min / median /
max per leg and each leg's ratio to the control of the same run.  One JSON line per measurement on stdout.

    python tools/gpu_histogram_rate.py [--N 1000000] [--steps 400] [--rounds 3]

``--kernels STEPS`` instead runs only the leg ``hist1`` with a sum probe of h beside it for that many steps:
the run to put under a kernel trace (``rocprofv3 --kernel-trace --stats -- python tools/gpu_histogram_rate.py
--kernels 200``) for the times of tfk_hist_partial and tfk_hist_final beside tfk_probe_partial (the histogram
kernels are not in the runtime's own timing table).  ``--kernels-leg cap256`` traces that leg instead.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np  # noqa: E402

from triflow_amd import Model, Simulation, schemes, workloads  # noqa: E402

LO, HI = 0.85, 1.15
HISTS = {"hist1": ("h", dict(bins=64, range=(LO, HI), every=1)),
         "hist10": ("h", dict(bins=64, range=(LO, HI), every=10)),
         "cap256": ("We * h * dxxxh", dict(bins=256, range=(-1e-4, 1e-4), every=1))}
LEGS = ("none", "hist1", "hist10", "cap256", "python1")
MODELS = {}


def make(N, mode):
    name, fields, pars, dt, _ = workloads.config_inputs(3, N)
    model = MODELS.setdefault(name, Model(*workloads.model_args(name)))
    sim = Simulation(model, fields, pars, dt=dt, scheme=schemes.ROS2, time_stepping=False)
    if mode in HISTS:
        expr, kw = HISTS[mode]
        sim.add_histogram("pdf", expr, **kw)
    elif mode == "python1":
        rows = []
        sim.add_post_process("python", lambda s: rows.append(
            np.histogram(np.asarray(s.fields["h"]), 64, (LO, HI))[0]))
    return sim


def drain(sim, mode):
    if mode in HISTS:
        sim.histograms                        # waits for the stream, fetches the rows
    else:
        b = sim.fields._device_backing()
        if b is not None:
            b.stepper.solver.sync()


def rate(N, mode, steps):
    sim = make(N, mode)
    for _ in range(5):
        next(sim)
    drain(sim, mode)
    n = steps if mode != "python1" else max(steps // 4, 20)
    t0 = time.perf_counter()
    for _ in range(n):
        next(sim)
    drain(sim, mode)
    return n / (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=10 ** 6)
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--kernels", type=int, default=0, metavar="STEPS")
    ap.add_argument("--kernels-leg", default="hist1", choices=sorted(HISTS))
    args = ap.parse_args()
    if args.kernels:
        sim = make(args.N, args.kernels_leg)
        sim.add_probe("sum_h", "h", reduce="sum")
        for _ in range(args.kernels):
            next(sim)
        t, edges, counts, outside = sim.histograms["pdf"]
        sim.probes
        assert (counts.sum(1) + outside.sum(1) == args.N).all()
        print(json.dumps(dict(what="kernels_run", leg=args.kernels_leg, N=args.N, steps=args.kernels,
                              rows=int(t.size), bins_hit=[int(np.count_nonzero(counts[0])),
                                                          int(np.count_nonzero(counts[-1]))],
                              outside_last=[int(v) for v in outside[-1]],
                              state_bytes_read_per_kernel=8 * args.N * 3)), flush=True)
        return
    rates = {mode: [] for mode in LEGS}
    for r in range(args.rounds):
        for mode in LEGS:
            v = rate(args.N, mode, args.steps)
            rates[mode].append(v)
            print(json.dumps(dict(what="steps_per_s", mode=mode, round=r, N=args.N, value=round(v, 1))), flush=True)
        print(json.dumps(dict(what="over_none", round=r, N=args.N,
                              **{k: round(rates[k][r] / rates["none"][r], 4) for k in LEGS if k != "none"})), flush=True)
    stats = {k: dict(min=round(min(v), 1), median=round(float(np.median(v)), 1), max=round(max(v), 1))
             for k, v in rates.items()}
    med = {k: s["median"] for k, s in stats.items()}
    print(json.dumps(dict(what="summary", N=args.N, steps_per_s=stats,
                          over_none={k: round(med[k] / med["none"], 4) for k in LEGS if k != "none"},
                          hist1_over_python1=round(med["hist1"] / med["python1"], 2))), flush=True)


if __name__ == "__main__":
    main()
