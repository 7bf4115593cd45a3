"""Device histograms: the distribution of the values of model expressions, counted where the state lives.

A histogram is a named expression in the model's own string language (what a probe accepts:
``observers.discretise``), a table of ``nbins + 1`` edges, a window of nodes (a slice) and a stride in steps
``every``.  With ``v`` the expression at the window's nodes, a row holds

* ``counts[i]``: the nodes with ``edges[i] <= v < edges[i + 1]``; the last bin also takes ``v == edges[-1]``;
* ``outside = (below, above, nan)``: the nodes with ``v < edges[0]``, ``v > edges[-1]`` and ``v != v``
  (``-inf`` / ``+inf`` go below / above; ``-0.0`` compares as ``0.0``),

so ``counts.sum() + outside.sum()`` is the number of window nodes in every row.  ``counts`` is
``np.histogram(v, bins=n, range=(lo, hi))[0]`` and ``np.histogram(v[~np.isnan(v)], bins=edges)[0]``, exactly:
they are integers, and a row does not depend on the order the nodes arrive in.  Uniform bins are given as a
number and a ``range``: the edges are ``np.linspace(lo, hi, bins + 1)``, computed on the host (what NumPy's
uniform fast path ends by comparing against).  There is no automatic range: it would take a min/max pass of
its own, and the rows of one series would have different edges.  Nothing is accumulated over time on the
device: that is ``counts.sum(0)`` on the host.

The expressions are lowered by ``codegen.lower_histograms`` and compiled into one more code object of the
model (``observers.py``: what the histograms share with the other observers), the only kind of code object
that holds the histogram kernels (``csrc/tf_histogram.h``); they read a resident state slot once per record
and write one row into the histogram's ring in device memory, which comes to the host when it is full and
when the series is read (``tf_histogram_*``).  Edges and window are data of the handle: histograms of the
same expressions share a code object whatever their edges, windows and strides.

:class:`HistogramSet` is what ``Simulation.add_histogram`` and ``Ensemble.add_histogram`` build on.
"""

import numpy as np

from . import codegen
from .observers import RowItem, RowObserverSet, _is_int, checked_capacity, checked_every, checked_nodes, discretise
from .observers import _Bound  # noqa: F401  (the tests build one)

__all__ = ["HistogramSet", "MAX_BINS", "DEFAULT_CAPACITY", "MAX_HISTOGRAMS", "bin_edges"]

#: bins of one histogram (TF_HIST_MAX_BINS of csrc/tf_args.h): a workgroup of tfk_hist_partial keeps the
#: edges and four sets of counters in LDS, 6 KiB at 256 bins
MAX_BINS = 256
#: rows of the device ring of a histogram: a run waits for the GPU once per this many records
DEFAULT_CAPACITY = 1024
#: histograms of one set (tf_histogram_create)
MAX_HISTOGRAMS = 64


def bin_edges(name, bins, range=None):
    """``bins`` and ``range`` of ``add_histogram`` -> float64 ``[nbins + 1]`` edges, or ``ValueError``."""
    if isinstance(bins, (bool, np.bool_)) or bins is None:
        raise ValueError("histogram %r: bins=%r, an integer 1 ... %d or a 1-D array of edges is expected"
                         % (name, bins, MAX_BINS))
    if isinstance(bins, str):
        raise ValueError("histogram %r: bins=%r: there is no automatic binning (it would take a min/max pass of "
                         "its own, and the rows of one series would have different edges): give the number of "
                         "bins and a range, or the edges" % (name, bins))
    if _is_int(bins):
        if bins < 1 or bins > MAX_BINS:
            raise ValueError("histogram %r: bins=%r, 1 ... %d bins per histogram" % (name, bins, MAX_BINS))
        if range is None:
            raise ValueError("histogram %r: bins=%d needs range=(lo, hi): there is no automatic range (it would "
                             "take a min/max pass of its own, and the rows of one series would have different "
                             "edges)" % (name, bins))
        try:
            lo, hi = range
            lo, hi = float(lo), float(hi)
        except (TypeError, ValueError):
            raise ValueError("histogram %r: range=%r, a pair (lo, hi) of numbers is expected" % (name, range))
        if not (np.isfinite(lo) and np.isfinite(hi)):
            raise ValueError("histogram %r: range=%r is not finite" % (name, range))
        if not lo < hi:
            raise ValueError("histogram %r: range=%r, lo < hi is expected" % (name, range))
        edges = np.linspace(lo, hi, int(bins) + 1)
        if not (np.diff(edges) > 0).all():
            raise ValueError("histogram %r: range=%r is too narrow for %d distinct bins" % (name, range, bins))
        return edges
    if range is not None:
        raise ValueError("histogram %r: range=%r goes with a number of bins, not with explicit edges"
                         % (name, range))
    try:
        edges = np.array(bins, dtype=float)
    except (TypeError, ValueError):
        raise ValueError("histogram %r: bins=%r, an integer 1 ... %d or a 1-D array of edges is expected"
                         % (name, bins, MAX_BINS))
    if edges.ndim != 1:
        raise ValueError("histogram %r: bins of %d dimensions, an integer or a 1-D array of edges is expected"
                         % (name, edges.ndim))
    if edges.size < 2 or edges.size > MAX_BINS + 1:
        raise ValueError("histogram %r: %d edges, 2 ... %d are expected (1 ... %d bins)"
                         % (name, edges.size, MAX_BINS + 1, MAX_BINS))
    if not np.isfinite(edges).all():
        raise ValueError("histogram %r: the edges are not all finite" % (name,))
    if not (np.diff(edges) > 0).all():
        raise ValueError("histogram %r: the edges are not strictly increasing" % (name,))
    return edges


class _Histogram(RowItem):
    def __init__(self, name, expression, disc, edges, every, window, capacity):
        super().__init__(name, expression, disc, every)    # (a row: [nsys][nbins + 3], int64)
        self.edges, self.window, self.capacity = edges, window, capacity

    @property
    def nbins(self):
        return self.edges.size - 1


class HistogramSet(RowObserverSet):
    """The histograms of one Simulation or Ensemble (``N`` nodes per system) and their series.

    Rows are recorded on the device (``record``) and fetched when the series are read (``series``):
    one ``tf_histogram`` handle per solver the set has run on, one code object per parameter layout /
    sweep segment of those solvers."""

    kind = "histogram"
    _laid_out = "the histogram windows were laid out for"

    # ---- the set ---------------------------------------------------------------------
    def add(self, name, expression, bins, range=None, every=1, nodes=slice(None), capacity=None):
        """Validate, lower and append one histogram (nothing is computed yet)."""
        if name in self.names:
            raise ValueError("a histogram named %r exists already" % (name,))
        every = checked_every("histogram", name, every)
        edges = bin_edges(name, bins, range)
        window = checked_nodes("histogram", name, nodes, self.N)
        capacity = checked_capacity("histogram", name, capacity)
        if len(self._items) >= MAX_HISTOGRAMS:
            raise ValueError("at most %d histograms per simulation (histogram %r)" % (MAX_HISTOGRAMS, name))
        disc = discretise(self.model, expression)
        codegen.lower_histograms(self.model, [disc])       # (what the C emitter refuses, refused now)
        self._flush()
        self._items.append(_Histogram(name, expression, disc, edges, every, window,
                                      DEFAULT_CAPACITY if capacity is None else capacity))
        self._reset()

    # ---- device side -----------------------------------------------------------------
    def _lower(self, mask):
        return codegen.lower_histograms(self.model, self.expressions(), parvec_mask=mask)

    def _make_handle(self, solver, code, spec):
        from ._capi import DeviceHistogram
        exprs = self.expressions()
        geometry = [(exprs.index(r.disc), r.nbins, r.capacity, *r.window) for r in self._items]
        return DeviceHistogram(solver, code, geometry, [r.edges for r in self._items], len(spec["host_consts"]))

    def _no_rows(self, r):
        return np.zeros((0, r.nsys, r.nbins + 3), dtype=np.int64)

    def series(self, per_system=True):
        """name -> (t [rows], edges [nbins + 1], counts [rows, nsys, nbins], outside [rows, nsys, 3]), int64
        counts (``per_system=False``: counts [rows, nbins], outside [rows, 3])."""
        self._flush()
        out = {}
        for r in self._items:
            c = self._rows(r) if per_system else self._rows(r)[:, 0]
            out[r.name] = (np.array(r.t, dtype=float), r.edges.copy(),
                           np.ascontiguousarray(c[..., :r.nbins]), np.ascontiguousarray(c[..., r.nbins:]))
        return out
