"""The model of ``burgers_upwind.py``, ``dU/dt = k dxxU - upwind(U, U, 2)`` in the exact mode of the step functions,
stepped explicitly: SSPRK3 at a CFL number of 0.4 of the initial state, ``dt = 0.4 dx / max|U|``.  The model is
not stiff at this resolution (``k dt / dx**2`` is 0.07 at the default N: the second-order upwind term at CFL 0.4
and this diffusion together stay inside SSPRK3's stability interval of 2.5), so the step is set by the advective
CFL limit and a linearly implicit scheme would pay for a factorisation it does not need: a step is three sweeps
of F, the last of which also writes the new state.  A device probe follows the steepest front."""
import sys

import numpy as np
from triflow_amd import Model, Simulation, schemes

N = int(sys.argv[1]) if len(sys.argv) > 1 else 2 ** 10
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 2000
CFL = 0.4
model = Model("k*dxxU - upwind(U, U, 2)", "U", ["k"], heaviside="exact")
x = np.linspace(0, 1, N, endpoint=False)
U0 = np.sin(2 * np.pi * x) + 0.2
fields = model.fields_template(x=x, U=U0)
pars = dict(k=2e-4, periodic=True)
dt = CFL * (1.0 / N) / np.abs(U0).max()

simul = Simulation(model, fields, pars, dt=dt, scheme=schemes.SSPRK3, time_stepping=False)
simul.add_probe("steepest", "-dxU", reduce="max")
for _ in range(steps):
    next(simul)

t, steepest = simul.probes["steepest"]
print("N = %d, dt = %.3e (CFL %.1f), k dt / dx^2 = %.3f" % (N, dt, CFL, pars["k"] * dt * N ** 2))
for row in range(0, t.size, max(t.size // 8, 1)):
    print("t = %.4f: steepest front %.2f" % (t[row], steepest[row]))
