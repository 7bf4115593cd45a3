"""Expression hooks at config 3 on a non-periodic grid (film model, N = 1e6, ROS2, fixed dt, Simulation loop):
steps/s
  none        no hook (control)
  dirichlet   DirichletHook at both ends
  open        the open-flow program: forced inlet, extrapolated outlet, sponge over the last 5 % of the nodes
  clip        the same plus the whole-field clip Max(h, 1e-6)
  py_open     `open` written as a Python callable (the generic path: the state goes through the host)
  py_clip     `clip` written as a Python callable
The legs are alternated in one process, ``--rounds`` times, blocks of ``--steps`` steps (the Python legs: a
quarter of that, 20 at least); min / median / max per leg and each leg's ratio to the control of the same
round.  One JSON line per measurement on stdout.

    python tools/gpu_hook_rate.py [--N 1000000] [--steps 400] [--rounds 3]

``--kernels STEPS`` instead runs only the leg ``clip`` with a sum probe of h beside it for that many steps:
the run to put under a kernel trace (``rocprofv3 --kernel-trace --stats -- python tools/gpu_hook_rate.py
--kernels 200``) for the times of tfk_hook_window and tfk_hook_points beside tfk_probe_partial (the hook
kernels are not in the runtime's own timing table).  ``--kernels-leg open`` traces that leg instead.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np  # noqa: E402

from triflow_amd import Model, Simulation, schemes, workloads  # noqa: E402

LEGS = ("none", "dirichlet", "open", "clip", "py_open", "py_clip")
MODELS = {}


# The data of config 3 have h = 1.1 and q = h**3 at both ends.  The boundary values start from them and the
# sponge's strength rises from zero with the cube of the distance into it: at dx = 1e-4 a jump of 1e-3
# between two nodes is a third derivative of 1e9, and a run that breaks down measures nothing.  The inlet
# is forced with an amplitude of 1e-12 for the same reason: the cost of a statement is not in its values.
def program(N, clip):
    w = N // 20                                   # the sponge: the last 5 % of the nodes, x = 95 ... 100
    st = [("h", 0, "1.1 + 1e-12 * sin(2 * pi * c * t)"),
          ("q", 0, "h * h * h"),
          ("h", -1, "at(h, -2)"),
          ("q", -1, "2 * at(q, -2) - at(q, -3)"),
          ("T", -1, "at(T, -2)"),
          ("h", slice(N - w, None), "h - k * ((x - 95) / 5)**3 * (h - 1.1)")]
    return st + ([("h", slice(None), "Max(h, 1e-6)")] if clip else [])


def python_hook(N, clip):
    w = N // 20

    def hook(t, fields, pars):
        h, q, T = fields["h"], fields["q"], fields["T"]
        h[0] = 1.1 + 1e-12 * np.sin(2 * np.pi * pars["c"] * t)
        q[0] = h[0] ** 3
        h[-1] = h[-2]
        q[-1] = 2 * q[-2] - q[-3]
        T[-1] = T[-2]
        h[N - w:] = h[N - w:] - pars["k"] * ((fields["x"][N - w:] - 95) / 5) ** 3 * (h[N - w:] - 1.1)
        if clip:
            h[:] = np.maximum(h, 1e-6)
        return fields, pars
    return hook


def make(N, mode):
    name, fields, pars, dt, _ = workloads.config_inputs(3, N)
    pars = dict(pars, periodic=False)
    model = MODELS.setdefault(name, Model(*workloads.model_args(name)))
    if mode == "none":
        hook = schemes.null_hook
    elif mode == "dirichlet":
        hook = schemes.DirichletHook(h={0: 1.1, -1: float(fields["h"][-1])},
                                     q={0: 1.1 ** 3, -1: float(fields["q"][-1])})
    elif mode in ("open", "clip"):
        hook = schemes.ExpressionHook(model, program(N, mode == "clip"))
    else:
        hook = python_hook(N, mode == "py_clip")
    return Simulation(model, fields, pars, dt=dt, scheme=schemes.ROS2, time_stepping=False, hook=hook)


def drain(sim):
    b = sim.fields._device_backing()
    if b is not None:
        b.stepper.solver.sync()


def rate(N, mode, steps):
    sim = make(N, mode)
    for _ in range(5):
        next(sim)
    drain(sim)
    n = steps if not mode.startswith("py_") else max(steps // 4, 20)
    t0 = time.perf_counter()
    for _ in range(n):
        next(sim)
    drain(sim)
    return n / (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=10 ** 6)
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--kernels", type=int, default=0, metavar="STEPS")
    ap.add_argument("--kernels-leg", default="clip", choices=("open", "clip"))
    args = ap.parse_args()
    if args.kernels:
        sim = make(args.N, args.kernels_leg)
        sim.add_probe("sum_h", "h", reduce="sum")
        for _ in range(args.kernels):
            next(sim)
        t, v = sim.probes["sum_h"]
        hook = sim._hook
        print(json.dumps(dict(what="kernels_run", leg=args.kernels_leg, N=args.N, steps=args.kernels,
                              rows=int(t.size), finite=bool(np.isfinite(v).all()),
                              launches_per_application=hook.launches(args.N), applications_per_step=3,
                              plane_bytes=8 * args.N, sponge_nodes=args.N // 20)), flush=True)
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
                          open_over_py_open=round(med["open"] / med["py_open"], 2),
                          clip_over_py_clip=round(med["clip"] / med["py_clip"], 2))), flush=True)


if __name__ == "__main__":
    main()
