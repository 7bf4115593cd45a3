"""Device statistics at config 3 (film model, N = 1e6, ROS2, fixed dt, Simulation loop): steps/s
  none        no statistic (control)
  mean1       the mean of h at every node, a sample per step
  var1        the variance of h at every node, a sample per step
  mean10      the mean of h, a sample every 10th step
  python1     the post-process that folds ``np.asarray(simul.fields["h"])`` into a running mean after every step
  python10    the same after every 10th step
The legs are alternated in one process, ``--rounds`` times, blocks of ``--steps`` steps; min / median /
max per leg.  Then the kernel time of tfk_stat (event stamps around the launches, tf_timing_*).
One JSON line per measurement on stdout.

    python tools/gpu_statistic_rate.py [--N 1000000] [--steps 400] [--rounds 3]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/gpu_statistic_rate.py --rounds 0   (kernel times only)
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np  # noqa: E402

from triflow_amd import Model, Simulation, schemes, workloads  # noqa: E402

STATISTICS = {"mean1": dict(every=1, stat="mean"), "var1": dict(every=1, stat="var"),
              "mean10": dict(every=10, stat="mean")}
LEGS = ("none", "mean1", "var1", "mean10", "python1", "python10")
MODELS = {}


def make(N, mode):
    name, fields, pars, dt, _ = workloads.config_inputs(3, N)
    model = MODELS.setdefault(name, Model(*workloads.model_args(name)))
    sim = Simulation(model, fields, pars, dt=dt, scheme=schemes.ROS2, time_stepping=False)
    if mode in STATISTICS:
        sim.add_statistic("s", "h", **STATISTICS[mode])
    elif mode.startswith("python"):
        every, acc = int(mode[len("python"):]), dict(k=0, m=np.zeros(N))

        def post(s):
            if s.i % every == 0:
                acc["k"] += 1
                acc["m"] += (np.asarray(s.fields["h"]) - acc["m"]) / acc["k"]
        sim.add_post_process("python", post)
    return sim


def drain(sim, mode):
    if mode in STATISTICS:
        sim.statistics                        # waits for the stream, fetches the planes
    else:
        b = sim.fields._device_backing()
        if b is not None:
            b.stepper.solver.sync()


def rate(N, mode, steps):
    sim = make(N, mode)
    for _ in range(5):
        next(sim)
    drain(sim, mode)
    n = steps if not mode.startswith("python") else max(steps // 4, 20)
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
    args = ap.parse_args()
    rates = {mode: [] for mode in LEGS}
    for r in range(args.rounds):
        for mode in LEGS:
            v = rate(args.N, mode, args.steps)
            rates[mode].append(v)
            print(json.dumps(dict(what="steps_per_s", mode=mode, round=r, N=args.N, value=round(v, 1))), flush=True)
    if args.rounds:
        stats = {k: dict(min=round(min(v), 1), median=round(float(np.median(v)), 1), max=round(max(v), 1))
                 for k, v in rates.items()}
        med = {k: s["median"] for k, s in stats.items()}
        print(json.dumps(dict(what="summary", N=args.N, steps_per_s=stats,
                              over_none={k: round(med[k] / med["none"], 4) for k in LEGS if k != "none"},
                              mean1_over_python1=round(med["mean1"] / med["python1"], 2),
                              mean10_over_python10=round(med["mean10"] / med["python10"], 2))), flush=True)

    # kernel time: event stamps around the statistic launches of 200 samples
    for mode in ("mean1", "var1"):
        sim = make(args.N, mode)
        next(sim)
        solver = sim.fields._device_backing().stepper.solver
        solver.timing(kernels=["tfk_stat"])
        solver.timing_reset()
        for _ in range(200):
            next(sim)
        sim.statistics
        rep = solver.timing_report()
        solver.timing(on=False)
        planes = 2 if mode == "var1" else 1
        print(json.dumps(dict(what="kernel_us", N=args.N, mode=mode,
                              per_launch_us={k: round(1e3 * ms / n, 2) for k, (ms, n) in rep.items()},
                              bytes_moved=8 * args.N * (3 + 2 * planes))), flush=True)


if __name__ == "__main__":
    main()
