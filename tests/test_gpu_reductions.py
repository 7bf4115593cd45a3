"""GPU suite of the step controllers' reductions (tests/reduction_cases.py) through libtriflow_hip.so and the gfx950
code objects: tfk_diffnorm and the host fold of its partials against an exact reference, the embedded Rosenbrock
estimate of tfk_vec_maxabs, the state plane I/O.  The CPU suite (tests/test_reductions.py) runs the same checks on
the emulation."""
import pytest

from tests import reduction_cases as rc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("nsys", [1, 3])
@pytest.mark.parametrize("name", rc.NORM_MODELS)
def test_diff_norms(name, nsys):
    rc.check_diff_norms(None, name, nsys)


@pytest.mark.parametrize("N,periodic", [(203, True), (203, False), (3001, True)])
def test_padding_after_steps(N, periodic):
    rc.check_padding_after_steps(None, N, periodic)


@pytest.mark.parametrize("name,nsys,N", rc.NONFINITE_CASES)
def test_nonfinite_norms(name, nsys, N):
    rc.check_nonfinite_norms(None, name, nsys, N)


def test_scheme_difference_norms():
    rc.check_scheme_difference_norms(None)


def test_estimate_against_oracle():
    rc.check_estimate_against_oracle(None)


def test_estimate_is_the_maximum_over_members():
    rc.check_estimate_is_the_maximum_over_members(None)


def test_estimate_queued_equals_blocking():
    rc.check_estimate_queued_equals_blocking(None)


def test_estimate_fused_update_switch():
    """... and the switch was really read: on the film model the fixed ROS2 step of the same two solvers has its
    update inside the back-substitution with TRIFLOW_FUSE_UPDATE=1 (no tfk_vec launch) and a tfk_vec launch
    with 0, as in test_state_update_inside_the_back_substitution."""
    reports = rc.check_estimate_fused_update_switch(None)
    film = [(fused, plain) for cid, _, fused, plain in reports if cid.startswith("film")]
    assert film
    for fused, plain in film:
        assert "tfk_vec" not in fused and plain["tfk_vec"][1] == 1, (sorted(fused), sorted(plain))


def test_estimate_nan_member():
    seen = rc.check_estimate_nan_member(None)
    assert all(how == rc.NAN_MEMBER_BEHAVIOUR[form] for (_, _, form), how in seen.items()), seen


def test_state_io():
    rc.check_state_io(None)
