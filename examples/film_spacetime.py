"""The space-time picture h(x, t) of the falling-film model (BASELINE config 3), recorded on the GPU:
1024 columns of a grid of 2**20 nodes, a row every 10 steps.  The state never leaves the device for it;
the series is saved as a container directory and read back with ``retrieve_container``."""
import sys
import tempfile

import numpy as np
from triflow_amd import Model, Simulation, schemes
from triflow_amd.container import retrieve_container
from triflow_amd.workloads import BENCH_MODELS

N = int(sys.argv[1]) if len(sys.argv) > 1 else 2 ** 20
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 200
model = Model(*BENCH_MODELS["M3_film"])
x = np.linspace(0, 100, N, endpoint=False)
h = 1 + 0.1 * np.cos(2 * np.pi * 4 * x / 100)
fields = model.fields_template(x=x, h=h, q=h ** 3, T=np.sin(2 * np.pi * x / 100))
pars = dict(c=1., eps=.5, We=.01, k=.05, periodic=True)

simul = Simulation(model, fields, pars, dt=1e-3, scheme=schemes.ROS2, time_stepping=False)
simul.add_recorder("h_xt", "h", every=10, nodes=slice(None, None, N // 1024))
simul.add_recorder("crest", "h", every=10, nodes=slice(None, None, N // 1024), pool="max")
for _ in range(steps):
    next(simul)

t, xc, values = simul.recorders["h_xt"]
print("h(x, t): %d rows x %d columns, t = %g ... %g, crest of the last row %.6f at x = %.3f"
      % (values.shape + (t[0], t[-1], simul.recorders["crest"][2][-1].max(), xc[np.argmax(values[-1])])))
path = simul.save_recorder("h_xt", tempfile.mkdtemp() + "/h_xt")
back = retrieve_container(path)
assert np.array_equal(back.data["h_xt"], values) and np.array_equal(back.data["t"], t)
print("saved to %s and read back: %s" % (path, {k: v.shape for k, v in back.data.items()}))
