"""The distribution of the film thickness of the falling-film model (BASELINE config 3): the PDF of h every
10 steps, counted on the GPU, and the median and the quartiles read off the counts.  The state never leaves
the device for it; a row is a few hundred bytes."""
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
simul.add_histogram("pdf", "h", bins=128, range=(0.8, 1.2), every=10)
for _ in range(steps):
    next(simul)

t, edges, counts, outside = simul.histograms["pdf"]
assert (counts.sum(1) + outside.sum(1) == N).all()   # every node is in a bin or in `outside`, in every row
print("%d rows, t = %g ... %g; outside the range (below, above, NaN): %s" % (t.size, t[0], t[-1], outside.sum(0)))


def quantile(row, q):
    """The q-quantile of a row, linear inside the bin where the cumulative count passes q * n."""
    cum = np.concatenate([[0], np.cumsum(row)])
    target = q * cum[-1]
    i = min(int(np.searchsorted(cum, target, side="right")) - 1, row.size - 1)
    frac = (target - cum[i]) / row[i] if row[i] else 0.0
    return edges[i] + frac * (edges[i + 1] - edges[i])


width = np.diff(edges)
for row in range(0, t.size, max(t.size // 8, 1)):
    pdf = counts[row] / (counts[row].sum() * width)          # a density: normalised on the host
    mode = int(np.argmax(pdf))
    print("t = %.3f: quartiles of h %.5f / %.5f / %.5f, most likely h in [%.4f, %.4f) (density %.2f)"
          % (t[row], quantile(counts[row], 0.25), quantile(counts[row], 0.5), quantile(counts[row], 0.75),
             edges[mode], edges[mode + 1], pdf[mode]))

# accumulated over time: a sum over the rows, on the host
total = counts.sum(0)
print("over the run: median h %.5f, fraction of (node, time) samples with h < 0.95: %.4f"
      % (quantile(total, 0.5), total[edges[1:] <= 0.95].sum() / total.sum()))
