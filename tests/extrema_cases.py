"""TEST-ONLY: the referee and the inputs the CPU and GPU tests of the device extrema share.

The referee is the rule of the extrema as written down, in NumPy with ``np.roll``: node ``g`` is a "max" iff
``v[g-1] < v[g]`` and ``v[g] > v[g+1]`` (a "min": both reversed), ``v[g]`` is finite and beyond the
threshold; the neighbours wrap, and on a grid that is not periodic nodes ``0`` and ``N - 1`` are struck
out.  Everything is compared exactly: the device stores only values it evaluated.
"""
import numpy as np


def referee(v, kind="max", periodic=True, threshold=None):
    """``(g [n], triples [n][3])``: the extrema of ``v [N]`` in ascending node order and ``(v[g-1], v[g],
    v[g+1])`` of each."""
    v = np.asarray(v, dtype=float)
    left, right = np.roll(v, 1), np.roll(v, -1)
    with np.errstate(invalid="ignore"):
        if kind == "max":
            is_ext = (left < v) & (v > right)
            if threshold is not None:
                is_ext &= v > threshold
        else:
            is_ext = (left > v) & (v < right)
            if threshold is not None:
                is_ext &= v < threshold
    is_ext &= np.isfinite(v)
    if not periodic:
        is_ext[0] = is_ext[-1] = False
    g = np.flatnonzero(is_ext)
    return g.astype(np.int64), np.stack([left[g], v[g], right[g]], axis=-1)


def refined(x, g, triples):
    """The vertex of the parabola through the three values, as the issue orders the operations."""
    x = np.asarray(x, dtype=float)
    dx = (x[-1] - x[0]) / (x.size - 1)
    vl, vc, vr = triples[:, 0], triples[:, 1], triples[:, 2]
    d = 0.5 * (vl - vr) / ((vl - vc) + (vr - vc))
    return x[g] + d * dx, vc - 0.25 * (vl - vr) * d


def assert_row(got, v, x, kind, periodic, threshold, max_count, refine, label=""):
    """One row ``got = (n, g [max_count], x [max_count], v [max_count])`` of a front end's series against the
    referee on the node values ``v``: everything exactly."""
    n, g, xs, vs = got
    rg, rt = referee(v, kind, periodic, threshold)
    assert n == rg.size, (label, n, rg.size)
    k = min(rg.size, max_count)
    assert g.shape == xs.shape == vs.shape == (max_count,), (label, g.shape)
    assert g.dtype == np.int64 and np.array_equal(g[:k], rg[:k]) and (g[k:] == -1).all(), label
    assert np.isnan(xs[k:]).all() and np.isnan(vs[k:]).all(), label
    if refine:
        rx, rv = refined(x, rg[:k], rt[:k])
    else:
        rx, rv = np.asarray(x, dtype=float)[rg[:k]], rt[:k, 1]
    assert xs[:k].tobytes() == rx.tobytes() and vs[:k].tobytes() == rv.tobytes(), label
    return k


def sawtooth(N):
    """1, 2, 1, 2 ...: every second node a crest, the others troughs."""
    return 1.0 + (np.arange(N) % 2)


def random_field(N, seed=5):
    return 1.0 + 0.1 * np.random.RandomState(seed).standard_normal(N)


def single_crest(N, at):
    """A ramp down on either side of node ``at`` (in the periodic sense): its only crest is ``at``; the
    only trough is half a turn away."""
    d = np.abs(np.arange(N) - at)
    return 2.0 - np.minimum(d, N - d) / float(N)
