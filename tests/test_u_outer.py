"""CPU suite of the factored outermost block of the stored pivot rows: the lowering, and the same kernel
bodies and host runtime through the emulation (tests/emu).  Checks and cases: tests/u_outer_cases.py; the GPU
suite (tests/test_gpu_u_outer.py) runs the comparison through the HIP path."""
import pytest

from tests import u_outer_cases as uc
from tests.emu.build_emu import EmuBackend


@pytest.fixture(scope="module")
def backend():
    return EmuBackend()


def test_film_form():
    uc.check_film_form()


def test_synthetic_form():
    uc.check_synth_form()


@pytest.mark.parametrize("name", uc.STORED_MODELS)
def test_stored_form_header_unchanged(name):
    uc.check_stored_form_header(name)


@pytest.mark.parametrize("respike", ["0", "1"])
@pytest.mark.parametrize("case", uc.FILM_GRID + uc.FILM_BDF2, ids=lambda c: c["id"])
def test_film_factored_against_stored(case, respike, backend):
    uc.check_factored_against_stored(backend, case, uc.FILM_TOL, TRIFLOW_L1_RESPIKE=respike)


@pytest.mark.parametrize("twist", ["0", "1"])
@pytest.mark.parametrize("case", uc.FILM_SWITCH, ids=lambda c: c["id"])
def test_film_twist(case, twist, backend):
    uc.check_factored_against_stored(backend, case, uc.FILM_TOL, TRIFLOW_L1_RESPIKE="1", TRIFLOW_L1_TWIST=twist)


@pytest.mark.parametrize("case", uc.FILM_SWITCH, ids=lambda c: c["id"])
def test_film_unfused_backsub(case, backend):
    uc.check_factored_against_stored(backend, case, uc.FILM_TOL, TRIFLOW_L1_FUSE_BACKSUB="0")


def test_film_short_chunks(backend):
    """4-node chunks on level 1: a plan of four levels"""
    uc.check_factored_against_stored(backend, uc.FILM_SWITCH[2], uc.FILM_TOL, TRIFLOW_M1="4")


def test_film_dense_mask(backend):
    """TRIFLOW_BLOCK_MASK=0: 6 + 1 < 9, the factored form with dense blocks"""
    uc.check_factored_against_stored(backend, uc.FILM_GRID[0], uc.FILM_TOL, TRIFLOW_BLOCK_MASK="0")
    uc.check_factored_against_stored(backend, uc.FILM_SWITCH[1], uc.FILM_TOL, TRIFLOW_BLOCK_MASK="0")


def test_stiff_keeps_stored_form(backend):
    uc.check_factored_against_stored(backend, uc.STIFF_CASE, uc.STIFF_TOL)


@pytest.mark.parametrize("periodic", [True, False], ids=["per", "clamp"])
@pytest.mark.parametrize("N, opts", [(203, dict(m1=4)), (203, {}), (2100, {})], ids=["203_m4", "203", "2100"])
def test_synthetic_solve(N, opts, periodic, backend):
    uc.check_synth_solve(backend, N, periodic, **opts)


@pytest.mark.parametrize("periodic", [True, False], ids=["per", "clamp"])
@pytest.mark.parametrize("N", [203, 2100])
def test_synthetic_solve_twisted(N, periodic, backend):
    """both walks store their half: the up direction of the synthetic model"""
    uc.check_synth_solve(backend, N, periodic, env=uc.SYNTH_TWIST)


def test_prebuilt_synthetic_model_is_the_tested_one():
    """build() pre-builds the code objects of SYNTH_MODEL for the GPU suite"""
    import __graft_entry__ as entry
    assert entry.U_OUTER_SYNTH == uc.SYNTH_MODEL
    assert "M3_film" in entry.PREBUILT_U_STORED
