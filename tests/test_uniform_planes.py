"""CPU suite of the write-once node-independent Jacobian planes: the same kernel bodies and host runtime
through the emulation (tests/emu).  Checks and cases: tests/uniform_planes_cases.py; the GPU suite
(tests/test_gpu_uniform_planes.py) runs the same ones through the HIP path."""
import pytest

from tests import uniform_planes_cases as uc
from tests.emu.build_emu import EmuBackend


@pytest.fixture(scope="module")
def backend():
    return EmuBackend()


@pytest.mark.parametrize("case", uc.TABLE_CASES, ids=lambda c: c[0])
def test_table_equality(case, backend):
    uc.check_table_equality(backend, case)


def test_invalidation_by_uploads(backend):
    uc.check_invalidation_by_uploads(backend)


def test_invalidation_restart(backend):
    uc.check_invalidation_restart(backend)


def test_nonuniform_models(backend):
    uc.check_nonuniform_models(backend)


def test_rescue_path(backend):
    uc.check_rescue_path(backend)


def test_graph_replay(backend):
    """(the emulation has no graphs: the launches are the eager ones -- the key logic runs on the GPU suite)"""
    uc.check_graph_replay(backend, N=600)


def test_step_doubling_trial(backend):
    uc.check_step_doubling_trial(backend)
