"""TEST-ONLY: the referee of the device histograms and the values that decide every tie.

``referee`` is the rule of ``triflow_amd/histograms.py`` written with comparisons only, one mask per bin;
``check_against_numpy`` holds it to both forms of ``np.histogram``.  ``adversarial`` places values on every
edge and one ulp to either side, with NaN, the infinities and both zeros."""
import numpy as np


def referee(v, edges):
    """``(counts [nbins], outside [3])`` int64 of the values ``v`` (any shape) for the edges ``edges``: bin
    ``i`` counts ``edges[i] <= v < edges[i + 1]``, the last bin also ``v == edges[-1]``; ``outside`` counts
    ``v < edges[0]``, ``v > edges[-1]`` and ``v != v``."""
    v = np.asarray(v, dtype=float).ravel()
    edges = np.asarray(edges, dtype=float)
    nbins = edges.size - 1
    with np.errstate(invalid="ignore"):
        counts = np.array([np.count_nonzero((edges[i] <= v) & (v < edges[i + 1])) for i in range(nbins)],
                          dtype=np.int64)
        counts[-1] += np.count_nonzero(v == edges[-1])
        outside = np.array([np.count_nonzero(v < edges[0]), np.count_nonzero(v > edges[-1]),
                            np.count_nonzero(v != v)], dtype=np.int64)
    assert counts.sum() + outside.sum() == v.size
    return counts, outside


def check_against_numpy(v, edges, uniform=None):
    """The referee's counts equal ``np.histogram(v[~isnan(v)], bins=edges)[0]`` and, with ``uniform = (n,
    lo, hi)`` whose ``np.linspace(lo, hi, n + 1)`` is ``edges``, ``np.histogram(v, bins=n, range=(lo, hi))[0]``
    (NumPy refuses a NaN only when it has to find the range itself, and infinities only there)."""
    v = np.asarray(v, dtype=float).ravel()
    counts, _ = referee(v, edges)
    assert np.array_equal(counts, np.histogram(v[~np.isnan(v)], bins=edges)[0])
    if uniform is not None:
        n, lo, hi = uniform
        assert np.array_equal(np.linspace(lo, hi, n + 1), edges)
        with np.errstate(invalid="ignore"):
            assert np.array_equal(counts, np.histogram(v, bins=n, range=(lo, hi))[0])
    return counts


def adversarial(edges):
    """Every edge and its two neighbours (``np.nextafter`` towards -inf and +inf), NaN, the infinities and
    both zeros, values in the middle of every bin and far outside."""
    edges = np.asarray(edges, dtype=float)
    mids = 0.5 * (edges[:-1] + edges[1:])
    return np.concatenate([edges, np.nextafter(edges, -np.inf), np.nextafter(edges, np.inf), mids,
                           [np.nan, np.inf, -np.inf, 0.0, -0.0, edges[0] - 1e300, edges[-1] + 1e300, np.nan]])


def cycled(values, N, seed=0):
    """A field of ``N`` nodes that cycles through ``values`` (every one of them is met when ``N >=
    len(values)``), shuffled so that neighbouring nodes fall into distant bins."""
    idx = np.arange(N) % len(values)
    np.random.RandomState(seed).shuffle(idx)
    return np.asarray(values, dtype=float)[idx]


def edge_sets(seed=0):
    """(edges, uniform or None): uniform bins of 1, 2, 64 and 256, ranges that include zero, and explicit
    edges that are far from uniform."""
    rs = np.random.RandomState(seed)
    out = []
    for n, lo, hi in ((1, 0.0, 3.0), (2, -1.0, 1.0), (64, 0.0, 3.0), (256, -0.7, 2.9), (7, -1e-3, 1e3)):
        out.append((np.linspace(lo, hi, n + 1), (n, lo, hi)))
    for n in (1, 2, 5, 64, 256):
        e = np.unique(np.concatenate([rs.uniform(-2.0, 2.0, n - n // 2), rs.standard_normal(n // 2 + 1) ** 3]))
        assert e.size == n + 1
        out.append((e, None))
    out.append((np.array([-1e300, -1.0, -5e-324, 0.0, 5e-324, 1.0, 1e300]), None))
    return out
