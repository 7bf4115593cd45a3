"""The ring of rows of the device spectra, extrema and histograms (RowRing, csrc/tf_solver.h) on the CPU,
through the host harness tests/ring_host: the emulation has no observer kernels, so nothing else in the CPU
suite runs this code.  Rows of 3 doubles, capacities 1 and 4, 17 and 50 rows: the ring wraps many times."""
import numpy as np
import pytest

from tests.ring_host import build_ring_host as host

WIDTH = 3
SIZES = [(1, 17), (1, 50), (4, 17), (4, 50)]


@pytest.fixture(scope="module")
def lib():
    return host.build()


@pytest.fixture
def ring(lib, request):
    r = host.Ring(lib, request.param, WIDTH)
    yield r
    r.close()


def rows(tags):
    """What ``fetch`` returns for the rows pushed with ``tags``, exactly."""
    return np.asarray(list(tags), dtype=float).reshape(-1, 1) + 0.25 * np.arange(WIDTH)


def push(ring, capacity, tags):
    """Every row lands at the next index of the ring, and the first one after a full ring at 0."""
    for tag in tags:
        before = ring.pending()
        at = ring.push(tag)
        assert 0 <= at < capacity
        assert ring.pending() == before + 1
        yield at


@pytest.mark.parametrize("ring, capacity, nrows", [(c, c, n) for c, n in SIZES], indirect=["ring"])
def test_small_rings_count_every_row_and_return_them_in_order(ring, capacity, nrows):
    assert ring.pending() == 0
    at = list(push(ring, capacity, range(nrows)))
    assert at == [i % capacity for i in range(nrows)]
    assert ring.pending() == nrows
    assert np.array_equal(ring.fetch(nrows), rows(range(nrows)))
    assert ring.pending() == 0


@pytest.mark.parametrize("ring, capacity, nrows", [(c, c, n) for c, n in SIZES], indirect=["ring"])
def test_staged_fetches_take_the_oldest_rows_and_leave_the_rest(ring, capacity, nrows):
    list(push(ring, capacity, range(nrows)))
    assert ring.fetch(0).shape == (0, WIDTH) and ring.pending() == nrows
    assert ring.fetch(-1).shape == (0, WIDTH) and ring.pending() == nrows
    assert np.array_equal(ring.fetch(1), rows([0])) and ring.pending() == nrows - 1
    fewer = nrows // 2
    assert np.array_equal(ring.fetch(fewer), rows(range(1, 1 + fewer))) and ring.pending() == nrows - 1 - fewer
    assert np.array_equal(ring.fetch(nrows + 7), rows(range(1 + fewer, nrows))) and ring.pending() == 0
    # an empty ring
    assert ring.fetch(5).shape == (0, WIDTH) and ring.pending() == 0
    # ... which goes on at row 0
    assert ring.push(99.0) == 0 and np.array_equal(ring.fetch(1), rows([99.0]))


@pytest.mark.parametrize("ring, capacity, nrows", [(c, c, n) for c, n in SIZES], indirect=["ring"])
def test_rows_drained_to_the_host_come_before_rows_still_in_the_ring(ring, capacity, nrows):
    first = nrows - 5
    list(push(ring, capacity, range(first)))
    assert np.array_equal(ring.fetch(3), rows(range(3)))           # (everything else is on the host now)
    assert ring.pending() == first - 3
    at = list(push(ring, capacity, range(first, first + 2)))       # two more, into the ring
    assert at == [i % capacity for i in range(2)]
    got = ring.fetch(first - 3 + 1)                                # the host's rows and one of the ring's
    assert np.array_equal(got, rows(range(3, first + 1)))
    assert ring.pending() == 1
    list(push(ring, capacity, range(first + 2, nrows)))
    assert ring.pending() == nrows - first - 1
    assert np.array_equal(ring.fetch(nrows), rows(range(first + 1, nrows)))
    assert ring.pending() == 0 and ring.fetch(1).shape == (0, WIDTH)
