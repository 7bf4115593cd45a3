"""A code object handed to the entry point of another kind on the MI355X: refused by name when the handle is
created, on the host, and the solver goes on."""
import numpy as np
import pytest

from oracle import corpus
from triflow_amd import Model, Simulation, codegen, compilers, probes, schemes
from triflow_amd._capi import DeviceModel, DeviceProbe

pytestmark = pytest.mark.gpu

N = 50


def _simulation(model):
    return Simulation(model, corpus.synthetic_fields("M2_diff", N), corpus.synthetic_pars("M2_diff", N, True),
                      dt=1e-3, scheme=schemes.Theta, time_stepping=False)


def test_a_code_object_of_another_kind_is_refused_when_the_handle_is_created():
    model = Model(*corpus.model_args("M2_diff"))
    sim = _simulation(model)
    next(sim)
    solver = sim.fields._device_backing().stepper.solver
    spec = solver.model.spec
    assert solver.N == N and solver.nsys == 1

    def code_of(kind, lower):
        block, _ = lower(model, [probes.discretise(model, "U")], parvec_mask=spec["parvec_mask"])
        with open(compilers.build_observer_code_object(model, block, kind, spec["parvec_mask"], spec["seg"],
                                                       spec["sweep_block"]), "rb") as f:
            return f.read()

    with pytest.raises(RuntimeError, match=r"kernel missing from code object: tfk_probe_partial\b"):
        DeviceProbe(solver, code_of("spectrum", codegen.lower_spectra), [0], 0)
    with pytest.raises(RuntimeError, match=r"kernel missing from code object: tfk_sweep_f\b"):
        DeviceModel(solver.lib, spec, code_of("histogram", codegen.lower_histograms))
    # the solver was not touched: its next Theta step is the one of a run that saw no refusal
    t, fields = next(sim)
    solver.sync()
    other = _simulation(model)
    next(other)
    t2, fields2 = next(other)
    got, want = np.asarray(fields["U"]), np.asarray(fields2["U"])
    assert t == t2 and np.isfinite(got).all() and got.tobytes() == want.tobytes()
