"""Explicit Runge-Kutta steps against the linearly implicit control on a non-stiff model (explicit
schemes): the Burgers model with ``upwind(U, U, 2)`` in exact mode, N = 1e6, periodic, fixed dt at CFL 0.4 of the
initial state, every block restarted from the initial state (400 steps cover 1e-4 of the ~0.16 it takes to
steepen); the viscosity is set so that k dt / dx**2 = 0.15 (k = 4.5e-7 at N = 1e6: the step is the
advective one).  Legs: ROS2 (control), then SSPRK3, RK4 and DOPRI5 with the fused last stage and with
``TRIFLOW_ERK_FUSED=0`` -- the switch is read when a solver is created, so every leg has a model, hence a solver,
of its own, made with the switch set for it.  The legs are alternated in blocks of ``--steps`` steps, ``--rounds``
times, in one process; min / median / max steps/s per leg, and the traffic of a step in units of one state's
planes by the count of :func:`traffic`.  One JSON line per block and a summary on stdout.

    python tools/gpu_explicit_rate.py [--N 1000000] [--steps 400] [--rounds 5] [--legs ROS2,SSPRK3,...]

Kernel times: the same command with ``--rounds 1`` under a kernel trace of its own.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np  # noqa: E402

from triflow_amd import Model, schemes  # noqa: E402
from triflow_amd.tableaux import ERK_TABLEAUX  # noqa: E402

EQUATION = ("k*dxxU - upwind(U, U, 2)", "U", ["k"])
CFL = 0.4


def inputs(N):
    x = np.linspace(0.0, 1.0, N, endpoint=False)
    U = np.sin(2 * np.pi * x) + 0.2
    dt = CFL * (1.0 / N) / np.abs(U).max()
    # (a viscosity the explicit schemes are stable with at this dt: k dt / dx**2 = 0.15 at every N)
    return dict(x=x, U=U), dict(k=0.15 / (dt * N ** 2), periodic=True), dt


def traffic(name, fused, with_err=False):
    """Planes of one state moved by a step: a stage reads U and the k_j of its non-zero a_ij and writes k_i;
    unfused, the update reads U and the k_j of the non-zero b_j and writes U+, the estimate reads the k_j
    of the non-zero d_j; fused, the last stage reads U and every k_j any of the three sums needs and writes
    U+ alone."""
    tab = ERK_TABLEAUX[name]
    s = len(tab.b)
    d = tab.b - tab.b_err if (with_err and tab.b_err is not None) else np.zeros(s)
    total = 0
    for i in range(s - 1 if fused else s):
        total += 2 + int(np.count_nonzero(tab.a[i]))
    if fused:
        need = (tab.a[s - 1] != 0) | (tab.b != 0) | (d != 0)
        return total + 2 + int(np.count_nonzero(need[:s - 1]))
    total += 2 + int(np.count_nonzero(tab.b))
    return total + int(np.count_nonzero(d))


class Leg:
    def __init__(self, name, N):
        self.name = name
        scheme, _, form = name.partition(":")
        saved = os.environ.get("TRIFLOW_ERK_FUSED")
        if form:
            os.environ["TRIFLOW_ERK_FUSED"] = "1" if form == "fused" else "0"
        try:
            self.model = Model(*EQUATION, heaviside="exact")
            self.fields, self.pars, self.dt = inputs(N)
            cls = getattr(schemes, scheme)
            self.scheme = cls(self.model, time_stepping=False) if scheme == "DOPRI5" else cls(self.model)
            self.block(5)                            # creates the solver, with the switch as set
        finally:
            if form:
                if saved is None:
                    del os.environ["TRIFLOW_ERK_FUSED"]
                else:
                    os.environ["TRIFLOW_ERK_FUSED"] = saved

    def block(self, steps):
        t, f = 0.0, self.model.fields_template(**self.fields)
        t, f = self.scheme(t, f, self.dt, self.pars)
        np.asarray(f["U"])[0]                        # uploaded and one step done: the clock starts here
        t0 = time.perf_counter()
        for _ in range(steps):
            t, f = self.scheme(t, f, self.dt, self.pars)
        last = np.asarray(f["U"])                    # waits for the queued steps
        rate = steps / (time.perf_counter() - t0)
        if not np.isfinite(last).all():
            raise RuntimeError("%s: the state is not finite after %d steps" % (self.name, steps))
        return rate


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=10 ** 6)
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--legs", default="ROS2,SSPRK3:fused,SSPRK3:unfused,RK4:fused,RK4:unfused,"
                                      "DOPRI5:fused,DOPRI5:unfused")
    args = ap.parse_args()
    legs = [Leg(name, args.N) for name in args.legs.split(",")]
    rates = {leg.name: [] for leg in legs}
    for r in range(args.rounds):
        for leg in legs:
            v = leg.block(args.steps)
            rates[leg.name].append(v)
            print(json.dumps(dict(what="block", leg=leg.name, round=r, N=args.N, steps_per_s=round(v, 1))), flush=True)
    summary = dict(what="summary", N=args.N, dt=legs[0].dt, steps=args.steps, legs={})
    for name, v in rates.items():
        scheme, _, form = name.partition(":")
        entry = dict(min=round(min(v), 1), median=round(float(np.median(v)), 1), max=round(max(v), 1))
        if form:
            entry["planes_per_step"] = traffic(scheme, form == "fused")
            entry["bytes_per_step"] = entry["planes_per_step"] * 8 * args.N
        summary["legs"][name] = entry
    for scheme in ("SSPRK3", "RK4", "DOPRI5"):
        if scheme + ":fused" in rates and scheme + ":unfused" in rates:
            summary[scheme + "_fused_over_unfused_time"] = round(
                float(np.median(rates[scheme + ":unfused"]) / np.median(rates[scheme + ":fused"])), 4)
    print(json.dumps(summary), flush=True)


if __name__ == "__main__":
    main()
