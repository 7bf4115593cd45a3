"""The exact mode of Heaviside / DiracDelta / Piecewise on the MI355X: F and J of the
gfx950 sweeps bit for bit against NumPy at every kink, the order of the linearised step, the five observers
through Simulation and Ensemble, the node-independent planes, and the compiler's resource report."""
import json
import os

import pytest

from tests import heaviside_cases as hc
from triflow_amd import codegen, compilers, probes

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", sorted(hc.MODELS))
def test_F_and_J_equal_numpy_bit_for_bit(name):
    for N in hc.MODEL_GRIDS:
        for periodic in (True, False):
            for per_node in (False, True):
                hc.check_FJ(name, None, N, periodic, per_node)


def test_the_linearised_step_is_third_order_only_in_exact_mode():
    hc.check_step_order(None, dts=(1e-3, 5e-4))


@pytest.mark.parametrize("N", hc.OBSERVER_GRIDS)
@pytest.mark.parametrize("periodic", [True, False], ids=["periodic", "clamped"])
def test_observers_through_a_simulation(N, periodic):
    for per_node in (False, True):
        hc.check_simulation_observers(N, periodic, per_node)


def test_observers_through_an_ensemble_of_three():
    hc.check_ensemble_observers()


def test_observers_of_a_default_mode_model_refuse():
    hc.check_default_mode_observers_refuse()


def test_uniform_planes_follow_the_sign_of_a_scalar_parameter():
    hc.check_uniform_planes_follow_a_scalar(None)


def _usage_of(hsaco):
    with open(hsaco[:-len(".hsaco")] + ".json") as f:
        return json.load(f)


@pytest.mark.parametrize("name", ["burgers_up", "pw"])
def test_model_code_objects_use_no_scratch_and_no_alternate_build(name):
    m = hc.model(name, "exact")
    for mask in (0, (1 << len(m._pars)) - 1):
        hsaco, _ = compilers.build_code_object(m, mask, seg=4)
        meta = _usage_of(hsaco)
        assert meta["kernels"] == compilers.resource_usage(hsaco) and len(meta["kernels"]) > 5
        spilled = {k: u["ScratchSize"] for k, u in meta["kernels"].items() if u.get("ScratchSize", 0) > 0}
        assert spilled == {} and meta["alt_kernels"] == [] and meta["alt_usage"] == {}, (name, spilled)
        assert compilers.alternate_of(hsaco) == (None, [])


def test_observer_code_objects_use_no_scratch():
    """The objects the five observers of the cases run from (one expression each, as their sets lower
    them; the solver's segment and block)."""
    m = hc.observer_model("exact")
    right, piece, step = ([probes.discretise(m, e)] for e in (hc.OBS_RIGHT, hc.OBS_PIECE, hc.OBS_STEP))
    for mask in (0, 2):
        blocks = dict(probe=codegen.lower_probes(m, right, ["integral"], parvec_mask=mask)[0],
                      record=codegen.lower_records(m, piece, parvec_mask=mask)[0],
                      stat=codegen.lower_statistics(m, step, parvec_mask=mask)[0],
                      spectrum=codegen.lower_spectra(m, step, parvec_mask=mask)[0],
                      extrema=codegen.lower_extrema(m, step, parvec_mask=mask)[0])
        for kind, block in blocks.items():
            assert "tf_heaviside" in block or "tf_select" in block
            hsaco = compilers.build_observer_code_object(m, block, kind, mask, 4, 256)
            meta = _usage_of(hsaco)
            mine = {k: u for k, u in meta["kernels"].items() if k.startswith("tfk_" + kind)}
            assert mine and all(u.get("ScratchSize", 0) == 0 for u in mine.values()), (kind, mine)
            assert meta["alt_kernels"] == [] and not os.path.exists(hsaco[:-len(".hsaco")] + ".alt.hsaco")
