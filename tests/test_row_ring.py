"""The rings of rows of the device observers (csrc/tf_solver.h) on the CPU, through the host harness
tests/ring_host: the emulation has no observer kernels, so nothing else in the CPU suite runs this code.

RowRing (probes, spectra, extrema, histograms): rows of 3 doubles, capacities 1 and 4, 17 and 50 rows: the
ring wraps many times.  HalfRing (recorders): the same scenarios at capacities 2 and 4 (halves of 1 and 2
rows), and two of its own.  A fetch empties a RowRing, whose next row is 0 again; a HalfRing goes on where it
is (``keeps_count``), so there the index is that of all the rows pushed so far.

Under the emulation the copies of a HalfRing are synchronous (an event is nothing, a queued copy is a
memcpy): these tests check the bookkeeping -- which row, which half, which page-locked buffer, what is
pending -- not the overlap of copies and records."""
import numpy as np
import pytest

from tests.ring_host import build_ring_host as host

WIDTH = 3
SIZES = [(1, 17), (1, 50), (4, 17), (4, 50)]
HALF_SIZES = [(2, 17), (2, 50), (4, 17), (4, 50)]
row_rings = pytest.mark.parametrize("ring, capacity, nrows", [(c, c, n) for c, n in SIZES], indirect=["ring"])
half_rings = pytest.mark.parametrize("half_ring, capacity, nrows", [(c, c, n) for c, n in HALF_SIZES],
                                     indirect=["half_ring"])


@pytest.fixture(scope="module")
def lib():
    return host.build()


@pytest.fixture
def ring(lib, request):
    r = host.Ring(lib, request.param, WIDTH)
    yield r
    r.close()


@pytest.fixture
def half_ring(lib, request):
    r = host.HalfRing(lib, request.param, WIDTH)
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


def first_index(ring, pushed):
    """Where the first row after a fetch lands (before the wrap) when ``pushed`` rows came before it."""
    return pushed if ring.keeps_count else 0


def count_every_row_and_return_them_in_order(ring, capacity, nrows):
    assert ring.pending() == 0
    at = list(push(ring, capacity, range(nrows)))
    assert at == [i % capacity for i in range(nrows)]
    assert ring.pending() == nrows
    assert np.array_equal(ring.fetch(nrows), rows(range(nrows)))
    assert ring.pending() == 0


def staged_fetches_take_the_oldest_rows_and_leave_the_rest(ring, capacity, nrows):
    list(push(ring, capacity, range(nrows)))
    assert ring.fetch(0).shape == (0, WIDTH) and ring.pending() == nrows
    assert ring.fetch(-1).shape == (0, WIDTH) and ring.pending() == nrows
    assert np.array_equal(ring.fetch(1), rows([0])) and ring.pending() == nrows - 1
    fewer = nrows // 2
    assert np.array_equal(ring.fetch(fewer), rows(range(1, 1 + fewer))) and ring.pending() == nrows - 1 - fewer
    assert np.array_equal(ring.fetch(nrows + 7), rows(range(1 + fewer, nrows))) and ring.pending() == 0
    # an empty ring
    assert ring.fetch(5).shape == (0, WIDTH) and ring.pending() == 0
    # ... which goes on at row 0 (a HalfRing: where it was)
    assert ring.push(99.0) == first_index(ring, nrows) % capacity and np.array_equal(ring.fetch(1), rows([99.0]))


def rows_drained_to_the_host_come_before_rows_still_in_the_ring(ring, capacity, nrows):
    first = nrows - 5
    list(push(ring, capacity, range(first)))
    assert np.array_equal(ring.fetch(3), rows(range(3)))           # (everything else is on the host now)
    assert ring.pending() == first - 3
    at = list(push(ring, capacity, range(first, first + 2)))       # two more, into the ring
    assert at == [(first_index(ring, first) + i) % capacity for i in range(2)]
    got = ring.fetch(first - 3 + 1)                                # the host's rows and one of the ring's
    assert np.array_equal(got, rows(range(3, first + 1)))
    assert ring.pending() == 1
    list(push(ring, capacity, range(first + 2, nrows)))
    assert ring.pending() == nrows - first - 1
    assert np.array_equal(ring.fetch(nrows), rows(range(first + 1, nrows)))
    assert ring.pending() == 0 and ring.fetch(1).shape == (0, WIDTH)


@row_rings
def test_small_rings_count_every_row_and_return_them_in_order(ring, capacity, nrows):
    count_every_row_and_return_them_in_order(ring, capacity, nrows)


@row_rings
def test_staged_fetches_take_the_oldest_rows_and_leave_the_rest(ring, capacity, nrows):
    staged_fetches_take_the_oldest_rows_and_leave_the_rest(ring, capacity, nrows)


@row_rings
def test_rows_drained_to_the_host_come_before_rows_still_in_the_ring(ring, capacity, nrows):
    rows_drained_to_the_host_come_before_rows_still_in_the_ring(ring, capacity, nrows)


@half_rings
def test_small_half_rings_count_every_row_and_return_them_in_order(half_ring, capacity, nrows):
    count_every_row_and_return_them_in_order(half_ring, capacity, nrows)


@half_rings
def test_half_ring_staged_fetches_take_the_oldest_rows_and_leave_the_rest(half_ring, capacity, nrows):
    staged_fetches_take_the_oldest_rows_and_leave_the_rest(half_ring, capacity, nrows)


@half_rings
def test_half_ring_rows_taken_to_the_host_come_before_rows_still_in_the_ring(half_ring, capacity, nrows):
    rows_drained_to_the_host_come_before_rows_still_in_the_ring(half_ring, capacity, nrows)


@pytest.mark.parametrize("half_ring, capacity", [(4, 4), (8, 8)], indirect=["half_ring"])
def test_half_ring_fetch_from_a_part_filled_half_then_fill_it(half_ring, capacity):
    """The rows at the start of a half that a fetch took (``lo``) are not copied again when the half fills:
    no row is lost, none comes twice, the order holds -- in the first round and after the ring has wrapped."""
    half, tag = capacity // 2, 0
    for _ in range(2):                                             # (second round: both halves were copied before)
        for part in range(1, half):                                # a fetch at 1 ... half - 1 rows of the first half
            list(push(half_ring, capacity, range(tag, tag + part)))
            assert np.array_equal(half_ring.fetch(capacity), rows(range(tag, tag + part)))
            assert half_ring.pending() == 0
            at = list(push(half_ring, capacity, range(tag + part, tag + half + 1)))    # fills it, and one more
            assert at == [i % capacity for i in range(tag + part, tag + half + 1)]
            assert half_ring.pending() == half + 1 - part
            # that one row is in the second half: fetched from a part-filled half too, which then fills
            assert np.array_equal(half_ring.fetch(capacity), rows(range(tag + part, tag + half + 1)))
            list(push(half_ring, capacity, range(tag + half + 1, tag + capacity)))
            assert half_ring.pending() == half - 1
            assert np.array_equal(half_ring.fetch(capacity), rows(range(tag + half + 1, tag + capacity)))
            assert half_ring.pending() == 0 and half_ring.fetch(1).shape == (0, WIDTH)
            tag += capacity


@pytest.mark.parametrize("half_ring, capacity, nrows", [(2, 2, 2), (2, 2, 3), (4, 4, 4), (4, 4, 5), (4, 4, 50)],
                         indirect=["half_ring"])
def test_half_ring_fetch_one_short_of_what_both_buffers_hold(half_ring, capacity, nrows):
    """Both page-locked buffers hold rows (from two halves on they do) and the caller's room is one row
    short: everything goes through the host's vector (the slow path), the oldest rows leave and the last one
    stays for the next fetch, in front of the rows recorded after it."""
    list(push(half_ring, capacity, range(nrows)))
    assert half_ring.pending() == nrows
    assert np.array_equal(half_ring.fetch(nrows - 1), rows(range(nrows - 1)))
    assert half_ring.pending() == 1
    at = list(push(half_ring, capacity, range(nrows, nrows + 2)))
    assert at == [i % capacity for i in range(nrows, nrows + 2)]
    assert np.array_equal(half_ring.fetch(3), rows(range(nrows - 1, nrows + 2)))
    assert half_ring.pending() == 0 and half_ring.fetch(1).shape == (0, WIDTH)
