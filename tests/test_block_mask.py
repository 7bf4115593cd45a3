"""CPU suite of the block mask of the banded solver: the same kernel bodies and host runtime through the
emulation (tests/emu).  Checks and cases: tests/block_mask_cases.py; the GPU suite
(tests/test_gpu_block_mask.py) runs the comparison through the HIP path."""
import pytest

from tests import block_mask_cases as bc
from tests.emu.build_emu import EmuBackend


@pytest.fixture(scope="module")
def backend():
    return EmuBackend()


@pytest.mark.parametrize("name", sorted(bc.MASK_MODELS))
def test_mask_contents(name):
    bc.check_mask_contents(name)


@pytest.mark.parametrize("respike", ["0", "1"])
@pytest.mark.parametrize("case", bc.FILM_CASES_CPU, ids=lambda c: c["id"])
def test_film_masked_against_dense(case, respike, backend):
    bc.check_masked_against_dense(backend, case, bc.FILM_TOL, TRIFLOW_L1_RESPIKE=respike)


@pytest.mark.parametrize("respike", ["0", "1"])
def test_stiff_masked_against_dense(respike, backend):
    """BDF2 with its Dirichlet hook"""
    bc.check_masked_against_dense(backend, bc.stiff_case("stiff_203", 203), bc.STIFF_TOL, TRIFLOW_L1_RESPIKE=respike)


@pytest.mark.parametrize("respike", ["0", "1"])
def test_film_bit_equality(respike, backend):
    """Pivots that stay inside their class: the skipped operations multiply exact zeros, the states of the
    masked and the dense kernels are the same bits."""
    bc.check_pivots_stay_in_class(bc.BIT_CASE)
    bc.check_masked_against_dense(backend, bc.BIT_CASE, bc.FILM_TOL, bit_equal=True, TRIFLOW_L1_RESPIKE=respike)


def test_cross_class_pivot(backend):
    bc.check_cross_class_pivot(backend)
