"""GPU suite of the wide memory phases of tfk_cr_factor (tests/cr_wide_io_cases.py): the default build
against -DTF_CR_WIDE_IO=0, bit for bit, and both against the oracle."""
import pytest

from tests import cr_wide_io_cases as wc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case,tol,env", wc.STEP_CASES, ids=[c[0]["id"] for c in wc.STEP_CASES])
def test_states_equal_bit_for_bit(case, tol, env):
    wc.check_steps(case, tol, env)


@pytest.mark.parametrize("name,N,opts,tol", wc.SOLVE_CASES,
                         ids=["%s_%d_%s" % (c[0], c[1], "_".join("%s%s" % kv for kv in sorted(c[2].items())))
                              for c in wc.SOLVE_CASES])
def test_factor_and_solve_equal_bit_for_bit(name, N, opts, tol):
    wc.check_solve(name, N, opts, tol)
