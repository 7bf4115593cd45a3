"""Viscous Burgers with the velocity itself upwinded, ``dU/dt = k dxxU - upwind(U, U, 2)``, in the exact mode of
the step functions: SymPy's Jacobian of ``Max(U, 0)`` / ``Min(U, 0)`` holds ``Heaviside(U)`` and
``Heaviside(-U)``, and ``heaviside="exact"`` evaluates them as written, so that J is the derivative of F and
ROS2 keeps its order (the default mode takes both as one, as the reference does).  A device probe integrates
``Heaviside(U)``: the length on which the flow runs to the right."""
import sys

import numpy as np
from triflow_amd import Model, Simulation, schemes

N = int(sys.argv[1]) if len(sys.argv) > 1 else 2 ** 16
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 400
model = Model("k*dxxU - upwind(U, U, 2)", "U", ["k"], heaviside="exact")
x = np.linspace(0, 1, N, endpoint=False)
fields = model.fields_template(x=x, U=np.sin(2 * np.pi * x) + 0.2)
pars = dict(k=1e-3, periodic=True)

simul = Simulation(model, fields, pars, dt=1e-3, scheme=schemes.ROS2, time_stepping=False)
simul.add_probe("right", "Heaviside(U)", reduce="integral")
simul.add_probe("momentum", "U", reduce="integral")
simul.add_probe("steepest", "-dxU", reduce="max")
for _ in range(steps):
    next(simul)

t, right = simul.probes["right"]
_, momentum = simul.probes["momentum"]
_, steepest = simul.probes["steepest"]
for row in range(0, t.size, max(t.size // 8, 1)):
    print("t = %.3f: flow to the right on %.4f of the domain, integral of U %.6f, steepest front %.1f"
          % (t[row], right[row], momentum[row], steepest[row]))
