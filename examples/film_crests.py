"""Follow the waves of the falling-film model (BASELINE config 3): the number of crests of the film thickness
over time and the celerity of the tallest one, from the crests found on the GPU every 10 steps.  The state
never leaves the device for it; a row is a few dozen numbers."""
import sys

import numpy as np
from triflow_amd import Model, Simulation, schemes
from triflow_amd.workloads import BENCH_MODELS

N = int(sys.argv[1]) if len(sys.argv) > 1 else 2 ** 20
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 400
length = 100.0
model = Model(*BENCH_MODELS["M3_film"])
x = np.linspace(0, length, N, endpoint=False)
h = 1 + 0.1 * np.cos(2 * np.pi * 4 * x / length) + 0.03 * np.cos(2 * np.pi * 7 * x / length)
fields = model.fields_template(x=x, h=h, q=h ** 3, T=np.sin(2 * np.pi * x / length))
pars = dict(c=1., eps=.5, We=.01, k=.05, periodic=True)

simul = Simulation(model, fields, pars, dt=1e-3, scheme=schemes.ROS2, time_stepping=False)
simul.add_extrema("crests", "h", kind="max", threshold=1.0, every=10, max_count=64)
for _ in range(steps):
    next(simul)

t, n, g, xc, vc = simul.extrema["crests"]
kept = np.minimum(n, xc.shape[1])                # entries of a row that hold a crest
print("%d rows, t = %g ... %g, crests above h = 1: %d ... %d" % (t.size, t[0], t[-1], n.min(), n.max()))
for row in range(0, t.size, max(t.size // 8, 1)):
    if kept[row] == 0:
        print("t = %.3f: no crest" % t[row])
        continue
    top = int(np.argmax(vc[row, :kept[row]]))
    print("t = %.3f: %d crests, the tallest h = %.6f at x = %.4f" % (t[row], n[row], vc[row, top], xc[row, top]))

# The celerity of the tallest crest of the first row: follow it from row to row and fit x(t).  The crest of
# the next row is the one nearest to where this one is expected -- its position plus the advance of the
# last interval -- by the signed distance around the periodic domain, so a crest that moves back a little is
# still the same crest; the path is kept unwrapped.
if kept[0] == 0:
    raise SystemExit("no crest above h = 1 in the first row: nothing to follow")
path, times, advance = [xc[0, int(np.argmax(vc[0, :kept[0]]))]], [t[0]], 0.0
for row in range(1, t.size):
    if kept[row] == 0:
        break                                    # the crest is gone: fit what there is
    signed = (xc[row, :kept[row]] - (path[-1] + advance) + length / 2) % length - length / 2
    step = advance + signed[int(np.argmin(np.abs(signed)))]
    path.append(path[-1] + step)
    times.append(t[row])
    advance = step
if len(path) > 1:
    celerity = np.polyfit(times, path, 1)[0]
    print("celerity of the tallest crest: %.4f (x from %.3f to %.3f, unwrapped, %d rows)"
          % (celerity, path[0], path[-1], len(path)))
