"""CPU suite of the step controllers' reductions -- the step-doubling difference norm, the embedded Rosenbrock
estimate, the state plane I/O they are measured through -- on the same kernel bodies and host runtime through the
emulation (tests/emu).  Checks and cases: tests/reduction_cases.py; the GPU suite (tests/test_gpu_reductions.py)
runs the same ones through the HIP path."""
import pytest

from tests import reduction_cases as rc
from tests.emu.build_emu import EmuBackend


@pytest.fixture(scope="module")
def backend():
    return EmuBackend()


@pytest.mark.parametrize("nsys", [1, 3])
@pytest.mark.parametrize("name", rc.NORM_MODELS)
def test_diff_norms(name, nsys, backend):
    rc.check_diff_norms(backend, name, nsys)


@pytest.mark.parametrize("N,periodic", [(203, True), (203, False), (3001, True)])
def test_padding_after_steps(N, periodic, backend):
    rc.check_padding_after_steps(backend, N, periodic)


@pytest.mark.parametrize("name,nsys,N", rc.NONFINITE_CASES)
def test_nonfinite_norms(name, nsys, N, backend):
    rc.check_nonfinite_norms(backend, name, nsys, N)


def test_scheme_difference_norms(backend):
    rc.check_scheme_difference_norms(backend)


def test_estimate_against_oracle(backend):
    rc.check_estimate_against_oracle(backend)


def test_estimate_is_the_maximum_over_members(backend):
    rc.check_estimate_is_the_maximum_over_members(backend)


def test_estimate_queued_equals_blocking(backend):
    rc.check_estimate_queued_equals_blocking(backend)


def test_estimate_fused_update_switch(backend):
    """Equal estimates and states with both values of the switch.  That the switch is read cannot show here: the
    update rides inside tfk_l1_fwd2_backsub (the re-elimination and the back-substitution as one launch, y in LDS),
    which only the HIP build has -- the emulation runs tfk_l1_fwd2 + tfk_l1_backsub_u and forms every new state in
    tfk_vec, with either value.  The GPU suite asserts 0 | 1 tfk_vec launches of the fixed step."""
    for cid, tname, fused, plain in rc.check_estimate_fused_update_switch(backend):
        for rep in (fused, plain):
            assert "tfk_l1_fwd2_backsub" not in rep and rep["tfk_vec"][1] == 1, (cid, tname, sorted(rep))


def test_estimate_nan_member(backend):
    seen = rc.check_estimate_nan_member(backend)
    assert all(how == rc.NAN_MEMBER_BEHAVIOUR[form] for (_, _, form), how in seen.items()), seen


def test_state_io(backend):
    rc.check_state_io(backend)
