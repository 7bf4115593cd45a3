"""Device spectra at config 3 (film model, N = 1e6, ROS2, fixed dt, Simulation loop): steps/s
  none        no spectrum (control)
  spec1       32 modes of h (1 ... 32), a row per step
  spec10      the same, a row every 10th step
  python1     the post-process ``np.fft.rfft(np.asarray(simul.fields["h"]))[:33]`` after every step
The legs are alternated in one process, ``--rounds`` times, blocks of ``--steps`` steps; min / median /
max per leg.  Then the kernel times of tfk_spectrum_partial and tfk_spectrum_final beside tfk_probe_partial
in the same run (event stamps around the launches, tf_timing_*).  One JSON line per measurement on stdout.

    python tools/gpu_spectrum_rate.py [--N 1000000] [--steps 400] [--rounds 3]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np  # noqa: E402

from triflow_amd import Model, Simulation, schemes, workloads  # noqa: E402

MODES = range(1, 33)
SPECTRA = {"spec1": 1, "spec10": 10}
LEGS = ("none", "spec1", "spec10", "python1")
MODELS = {}


def make(N, mode):
    name, fields, pars, dt, _ = workloads.config_inputs(3, N)
    model = MODELS.setdefault(name, Model(*workloads.model_args(name)))
    sim = Simulation(model, fields, pars, dt=dt, scheme=schemes.ROS2, time_stepping=False)
    if mode in SPECTRA:
        sim.add_spectrum("s", "h", modes=MODES, every=SPECTRA[mode])
    elif mode == "python1":
        rows = []
        sim.add_post_process("python", lambda s: rows.append(np.fft.rfft(np.asarray(s.fields["h"]))[:33]))
    return sim


def drain(sim, mode):
    if mode in SPECTRA:
        sim.spectra                           # waits for the stream, fetches the rows
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
                              spec1_over_python1=round(med["spec1"] / med["python1"], 2))), flush=True)

    # kernel times: event stamps around the launches of 200 records, a sum probe of h in the same run
    sim = make(args.N, "spec1")
    sim.add_probe("sum_h", "h", reduce="sum")
    next(sim)
    solver = sim.fields._device_backing().stepper.solver
    kernels = ["tfk_spectrum_partial", "tfk_spectrum_final", "tfk_probe_partial", "tfk_probe_final"]
    solver.timing(kernels=kernels)
    solver.timing_reset()
    for _ in range(200):
        next(sim)
    sim.spectra, sim.probes
    rep = solver.timing_report()
    solver.timing(on=False)
    print(json.dumps(dict(what="kernel_us", N=args.N, modes=len(MODES),
                          per_launch_us={k: round(1e3 * ms / n, 2) for k, (ms, n) in rep.items() if n},
                          state_bytes_read=8 * args.N * 3)), flush=True)


if __name__ == "__main__":
    main()
