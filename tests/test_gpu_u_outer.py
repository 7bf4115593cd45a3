"""GPU suite of the factored outermost block of the stored pivot rows (tests/u_outer_cases.py) through
libtriflow_hip.so and the gfx950 code objects: the factored form against the stored one (TRIFLOW_U_OUTER=0)
and the oracle.

N = 2100 with 4-node chunks on level 1 is a plan of four levels (tfk_l1_solve_cr and
tfk_l1_fwd2_backsub_cr run); N = 40 000 with the default plan takes the split two-wavefront factorisation
walk, the twisted fused back-substitution, the update inside it and the fused level-2 launches."""
import pytest

from tests import u_outer_cases as uc

pytestmark = pytest.mark.gpu


def _env(case):
    return dict(TRIFLOW_M1="4") if case["N"] == 2100 else {}


@pytest.mark.parametrize("respike", ["0", "1"])
@pytest.mark.parametrize("case", uc.FILM_GRID + uc.FILM_BDF2, ids=lambda c: c["id"])
def test_film_factored_against_stored(case, respike):
    uc.check_factored_against_stored(None, case, uc.FILM_TOL, TRIFLOW_L1_RESPIKE=respike, **_env(case))


@pytest.mark.parametrize("twist", ["0", "1"])
@pytest.mark.parametrize("case", uc.FILM_SWITCH, ids=lambda c: c["id"])
def test_film_twist(case, twist):
    uc.check_factored_against_stored(None, case, uc.FILM_TOL, TRIFLOW_L1_RESPIKE="1", TRIFLOW_L1_TWIST=twist,
                                     **_env(case))


@pytest.mark.parametrize("case", uc.FILM_SWITCH, ids=lambda c: c["id"])
def test_film_unfused_backsub(case):
    uc.check_factored_against_stored(None, case, uc.FILM_TOL, TRIFLOW_L1_FUSE_BACKSUB="0", **_env(case))


def test_film_dense_mask():
    uc.check_factored_against_stored(None, uc.FILM_SWITCH[1], uc.FILM_TOL, TRIFLOW_BLOCK_MASK="0")


def test_film_large():
    uc.check_factored_against_stored(None, uc.FILM_LARGE, uc.FILM_TOL)


@pytest.mark.parametrize("periodic", [True, False], ids=["per", "clamp"])
@pytest.mark.parametrize("N, opts", [(203, dict(m1=4)), (2100, {})], ids=["203_m4", "2100"])
def test_synthetic_solve(N, opts, periodic):
    uc.check_synth_solve(None, N, periodic, **opts)


@pytest.mark.parametrize("periodic", [True, False], ids=["per", "clamp"])
@pytest.mark.parametrize("N", [203, 2100])
def test_synthetic_solve_twisted(N, periodic):
    """both walks store their half: the up direction of the synthetic model"""
    uc.check_synth_solve(None, N, periodic, env=uc.SYNTH_TWIST)
