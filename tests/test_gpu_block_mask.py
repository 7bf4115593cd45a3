"""GPU suite of the block mask of the banded solver (tests/block_mask_cases.py) through libtriflow_hip.so
and the gfx950 code objects: the masked kernels against the dense ones (TRIFLOW_BLOCK_MASK=0) and the oracle.

N = 2100 with 4-node chunks on level 1 is a plan of four levels (tfk_l1_solve_cr and
tfk_l1_fwd2_backsub_cr run); N = 40 000 with the default plan takes the split two-wavefront factorisation
walk, the twisted fused back-substitution and the update inside the back-substitution."""
import pytest

from tests import block_mask_cases as bc

pytestmark = pytest.mark.gpu

FILM_CASES = [bc.film_case("gpu_film_%d_%s_%dm" % (N, "per" if periodic else "clamp_hook", nsys), N, periodic, nsys,
                           "ROS2", hook=None if periodic else "film")
              for N in (2100, 40000) for periodic in (True, False) for nsys in (1, 3)]


@pytest.mark.parametrize("case", FILM_CASES, ids=lambda c: c["id"])
def test_film_masked_against_dense(case):
    env = dict(TRIFLOW_M1="4") if case["N"] == 2100 else {}
    bc.check_masked_against_dense(None, case, bc.FILM_TOL, **env)


def test_stiff_masked_against_dense():
    bc.check_masked_against_dense(None, bc.stiff_case("gpu_stiff_4000", 4000), bc.STIFF_TOL)
