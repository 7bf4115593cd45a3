"""The falling-film model (BASELINE config 3) as an open flow: a forced inlet, an extrapolated outlet and a
sponge layer in front of it, written as an ExpressionHook -- a program of statements in the model's own
language that two kernels run on the state where it lives, at the places and with the times the reference
calls ``hook`` -- with a recorder on the run.  The state never comes to the host."""
import sys

import numpy as np
from triflow_amd import Model, Simulation, schemes
from triflow_amd.workloads import BENCH_MODELS

N = int(sys.argv[1]) if len(sys.argv) > 1 else 2 ** 18
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 400
length = 100.0
model = Model(*BENCH_MODELS["M3_film"])
x = np.linspace(0, length, N)
h = np.ones(N)
fields = model.fields_template(x=x, h=h, q=h ** 3 / 3, T=np.zeros(N))
pars = dict(c=1., eps=.5, We=.01, k=.05, periodic=False)

sponge = N // 20                                   # the last 5 % of the nodes
hook = schemes.ExpressionHook(model, [
    ("h", 0, "1 + 0.05 * sin(2 * pi * 2 * t)"),              # the inlet is forced at frequency 2
    ("q", 0, "h * h * h / 3"),                               # the flat-film flux of the h[0] just written
    ("h", -1, "at(h, -2)"),                                  # outflow: a copy of the node before
    ("q", -1, "2 * at(q, -2) - at(q, -3)"),                  # linear extrapolation
    ("T", -1, "at(T, -2)"),
    ("h", slice(N - sponge, None), "h - k * (h - 1)"),       # the sponge relaxes h towards the flat film
    ("h", slice(None), "Max(h, 1e-6)"),                      # the film never dries out
])
print("%d statements, %d launches per application, idempotent: %s"
      % (len(hook.statements), hook.launches(N), hook.idempotent))

simul = Simulation(model, fields, pars, dt=1e-3, scheme=schemes.ROS2, time_stepping=False, hook=hook)
simul.add_recorder("h_xt", "h", every=max(steps // 40, 1), nodes=slice(None, None, max(N // 512, 1)))
for _ in range(steps):
    next(simul)

t, xr, values = simul.recorders["h_xt"]
print("%d rows of %d columns, t = %g ... %g" % (values.shape[0], values.shape[1], t[0], t[-1]))
for row in range(0, t.size, max(t.size // 8, 1)):
    crest = int(np.argmax(values[row]))
    print("t = %.3f: inlet h %.5f, highest crest %.5f at x = %.2f, outlet h %.5f"
          % (t[row], values[row, 0], values[row, crest], xr[crest], values[row, -1]))
