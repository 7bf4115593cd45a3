"""Device probes at config 3 (film model, N = 1e6, ROS2, fixed dt, Simulation loop): steps/s
without probes, with three probes recorded after every step (integral, max, argmax of h), and with
the equivalent Python post-process on ``simul.fields`` (np.trapz / max / argmax: the state goes
to the host and back every step).  The three are alternated, ``--rounds`` times.  Then the kernel
times of tfk_probe_partial / tfk_probe_final (event stamps around the launches, tf_timing_*) and
the algorithmic bytes over kernel time.  One JSON line per measurement on stdout.

    python tools/gpu_probe_rate.py [--N 1000000] [--steps 400] [--rounds 3]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/gpu_probe_rate.py --rounds 0   (kernel times only)
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np  # noqa: E402

from triflow_amd import Model, Simulation, schemes, workloads  # noqa: E402

PROBES = [("mass", "h", "integral"), ("crest", "h", "max"), ("where", "h", "argmax")]


def make(N, mode):
    name, fields, pars, dt, _ = workloads.config_inputs(3, N)
    model = MODELS.setdefault(name, Model(*workloads.model_args(name)))
    sim = Simulation(model, fields, pars, dt=dt, scheme=schemes.ROS2, time_stepping=False)
    if mode == "probes":
        for p in PROBES:
            sim.add_probe(*p)
    elif mode == "python":
        out = []

        def post(s):
            x, h = np.asarray(s.fields["x"]), np.asarray(s.fields["h"])
            out.append((s.t, np.trapezoid(h, x) if hasattr(np, "trapezoid") else np.trapz(h, x), h.max(), x[np.argmax(h)]))
        sim.add_post_process("python", post)
    return sim


def drain(sim, mode):
    if mode == "probes":
        sim.probes                            # waits for the stream, fetches the rows
    else:
        b = sim.fields._device_backing()
        if b is not None:
            b.stepper.solver.sync()


def rate(N, mode, steps):
    sim = make(N, mode)
    for _ in range(5):
        next(sim)
    drain(sim, mode)
    n = steps if mode != "python" else max(steps // 10, 20)
    t0 = time.perf_counter()
    for _ in range(n):
        next(sim)
    drain(sim, mode)
    return n / (time.perf_counter() - t0)


MODELS = {}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=10 ** 6)
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    rates = {"none": [], "probes": [], "python": []}
    for r in range(args.rounds):
        for mode in ("none", "probes", "python"):
            v = rate(args.N, mode, args.steps)
            rates[mode].append(v)
            print(json.dumps(dict(what="steps_per_s", mode=mode, round=r, N=args.N, value=round(v, 1))), flush=True)
    if args.rounds:
        med = {k: float(np.median(v)) for k, v in rates.items()}
        print(json.dumps(dict(what="summary", N=args.N, median_steps_per_s=med,
                              probes_over_none=round(med["probes"] / med["none"], 4),
                              python_over_none=round(med["python"] / med["none"], 4))), flush=True)

    # kernel time: event stamps around the probe launches of 200 records
    sim = make(args.N, "probes")
    next(sim)
    solver = sim.fields._device_backing().stepper.solver
    solver.timing(kernels=["tfk_probe_partial", "tfk_probe_final"])
    solver.timing_reset()
    for _ in range(200):
        next(sim)
    sim.probes
    rep = solver.timing_report()
    solver.timing(on=False)
    nbytes = 8 * 3 * args.N                   # (nvar + nh + vector parameters) * N doubles read
    out = {}
    for k, (ms, n) in rep.items():
        out[k] = round(1e3 * ms / n, 2)
    part = out.get("tfk_probe_partial")
    print(json.dumps(dict(what="kernel_us", N=args.N, probes=len(PROBES), per_launch_us=out,
                          algorithmic_bytes=nbytes,
                          partial_TBps=round(nbytes / (part * 1e-6) / 1e12, 2) if part else None)), flush=True)


if __name__ == "__main__":
    main()
