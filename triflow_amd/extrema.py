"""Device extrema: the crests and troughs of model expressions, found where the state lives.

An extrema observer is a named expression in the model's own string language (what a probe accepts:
``observers.discretise``), a kind ("max" or "min"), an optional threshold, a stride in steps ``every`` and
the number of entries of a row, ``max_count``.  With ``v`` the expression at the nodes ``0 ... N - 1`` of a
system, node ``g`` is an extremum of kind "max" iff ``v[g-1] < v[g]`` and ``v[g] > v[g+1]``, both strictly
("min": both reversed), ``v[g]`` is finite and, with a threshold, ``v[g] > threshold`` ("min": ``<``).  On
a periodic grid the neighbours wrap; on any other grid nodes ``0`` and ``N - 1`` are never extrema:
``scipy.signal.argrelextrema(v, np.greater, mode="wrap")`` (``np.less``; ``mode="clip"``).  A NaN compares
false, so a NaN disqualifies its neighbours.  A plateau of exactly equal values is not reported: neither
of two equal neighbours is strictly above the other.

A row is ``n``, the number of extrema found (it may exceed ``max_count``), and the first ``min(n,
max_count)`` of them in ascending node order: the node ``g``, a position ``x`` and a value ``v``.  The
device stores the node and the three values ``(v[g-1], v[g], v[g+1])`` it evaluated; with ``refine=True``
the host puts the vertex of the parabola through them into ``x`` and ``v``, with ``refine=False`` the
node's own ``x`` and ``v[g]``.  The expressions are lowered by ``codegen.lower_extrema`` and compiled into
one more code object of the model (``observers.py``: what the extrema share with the other observers);
the kernels (``csrc/tf_extrema.h``) read a resident state slot twice per record -- count, integer scan,
scatter -- and write one row into the observer's ring in device memory, which comes to the host when it is
full and when the series is read (``tf_extrema_*``).  Kind, threshold, ``max_count`` and ``every`` are
launch arguments: sets that differ only in them share a code object.

:class:`ExtremaSet` is what ``Simulation.add_extrema`` and ``Ensemble.add_extrema`` build on.
"""

import numpy as np

from . import codegen
from .observers import RowItem, RowObserverSet, _is_int, checked_capacity, checked_every, discretise
from .observers import _Bound  # noqa: F401  (the tests build one)

__all__ = ["ExtremaSet", "EXTREMA_KINDS", "MAX_COUNT", "DEFAULT_MAX_COUNT", "MAX_EXTREMA", "refine_parabola"]

#: kinds of extrema (TF_EXT_MAX, TF_EXT_MIN of csrc/tf_args.h: same order)
EXTREMA_KINDS = ("max", "min")
#: entries of one row at most (TF_EXT_MAX_COUNT of csrc/tf_args.h)
MAX_COUNT = 8192
DEFAULT_MAX_COUNT = 256
#: observers of one set (tf_extrema_create)
MAX_EXTREMA = 64


def refine_parabola(xg, dx, vl, vc, vr):
    """The vertex ``(x, v)`` of the parabola through ``(xg - dx, vl), (xg, vc), (xg + dx, vr)``.  The
    strict inequalities of an extremum make the denominator non-zero."""
    d = 0.5 * (vl - vr) / ((vl - vc) + (vr - vc))
    return xg + d * dx, vc - 0.25 * (vl - vr) * d


class _Extrema(RowItem):
    def __init__(self, name, expression, disc, kind, threshold, every, max_count, capacity, refine):
        super().__init__(name, expression, disc, every)    # (a row: [nsys][1 + 4 * max_count])
        self.kind, self.threshold = kind, threshold
        self.max_count, self.capacity, self.refine = max_count, capacity, refine
        self.x = None                # [nsys][N]: the nodes' coordinates at the first row

    def device_threshold(self):
        if self.threshold is not None:
            return self.threshold
        return -np.inf if self.kind == "max" else np.inf


class ExtremaSet(RowObserverSet):
    """The extrema observers of one Simulation or Ensemble (``N`` nodes per system) and their series.

    Rows are recorded on the device (``record``) and fetched when the series are read (``series``):
    one ``tf_extrema`` handle per solver the set has run on, one code object per parameter layout /
    sweep segment of those solvers."""

    kind = "extrema"
    _laid_out = "the extrema were laid out for"

    # ---- the set ---------------------------------------------------------------------
    def add(self, name, expression, kind="max", threshold=None, every=1, max_count=DEFAULT_MAX_COUNT,
            capacity=None, refine=True):
        """Validate, lower and append one observer (nothing is computed yet)."""
        if name in self.names:
            raise ValueError("an extrema observer named %r exists already" % (name,))
        if kind not in EXTREMA_KINDS:
            raise ValueError("extrema %r: kind=%r, one of %s is expected" % (name, kind, ", ".join(EXTREMA_KINDS)))
        if threshold is not None:
            if isinstance(threshold, (bool, np.bool_)) or not isinstance(threshold, (int, float, np.integer, np.floating)) \
                    or not np.isfinite(threshold):
                raise ValueError("extrema %r: threshold=%r, a finite number or None is expected" % (name, threshold))
            threshold = float(threshold)
        every = checked_every("extrema", name, every)
        if not _is_int(max_count) or not 1 <= max_count <= MAX_COUNT:
            raise ValueError("extrema %r: max_count=%r, an integer in 1 ... %d is expected" % (name, max_count, MAX_COUNT))
        capacity = checked_capacity("extrema", name, capacity)
        if self.N < 3:
            raise ValueError("extrema %r: a grid of N=%d nodes, an extremum has two neighbours (N >= 3)" % (name, self.N))
        if len(self._items) >= MAX_EXTREMA:
            raise ValueError("at most %d extrema observers per simulation (extrema %r)" % (MAX_EXTREMA, name))
        disc = discretise(self.model, expression)
        codegen.lower_extrema(self.model, [disc])          # (what the C emitter refuses, refused now)
        self._flush()
        self._items.append(_Extrema(name, expression, disc, kind, threshold, every, int(max_count), capacity,
                                    bool(refine)))
        self._reset()

    # ---- device side -----------------------------------------------------------------
    def _lower(self, mask):
        return codegen.lower_extrema(self.model, self.expressions(), parvec_mask=mask)

    def _make_handle(self, solver, code, spec):
        from ._capi import DeviceExtrema
        exprs = self.expressions()
        geometry = [(exprs.index(r.disc), EXTREMA_KINDS.index(r.kind), r.max_count, r.capacity or 0)
                    for r in self._items]
        return DeviceExtrema(solver, code, geometry, [r.device_threshold() for r in self._items],
                             len(spec["host_consts"]))

    def _first_row(self, r, x, solver):
        r.x = np.array(np.broadcast_to(x, (solver.nsys, self.N)))

    def _no_rows(self, r):
        return np.zeros((0, r.nsys, 1 + 4 * r.max_count))

    @staticmethod
    def rows_of(raw, x, refine):
        """The device's rows ``raw [rows][nsys][1 + 4 * max_count]`` -> ``(n, g, x, v)``: ``n [rows][nsys]``
        int64, ``g`` int64 (-1 past ``min(n, max_count)``), ``x`` and ``v`` float64 (NaN there).
        ``x [nsys][N]``: the nodes' coordinates."""
        rows, nsys, width = raw.shape
        mc = (width - 1) // 4
        n = raw[:, :, 0].astype(np.int64)
        ent = raw[:, :, 1:].reshape(rows, nsys, mc, 4)
        kept = np.arange(mc)[None, None, :] < np.minimum(n, mc)[:, :, None]
        g = np.where(kept, ent[..., 0], -1.0).astype(np.int64)
        vl, vc, vr = (np.where(kept, ent[..., j], np.nan) for j in (1, 2, 3))
        gi = np.where(kept, g, 0)
        xg = x[np.arange(nsys)[None, :, None], gi] if rows else np.zeros((0, nsys, mc))
        xg = np.where(kept, xg, np.nan)
        if not refine:
            return n, g, xg, vc
        dx = ((x[:, -1] - x[:, 0]) / (x.shape[1] - 1))[None, :, None]
        with np.errstate(all="ignore"):
            xr, vv = refine_parabola(xg, dx, vl, vc, vr)
        return n, g, xr, vv

    def series(self, per_system=True):
        """name -> (t [rows], n [rows, nsys], g, x, v [rows, nsys, max_count]) (``per_system=False``: n
        [rows], g, x, v [rows, max_count])."""
        self._flush()
        out = {}
        for r in self._items:
            x = np.zeros((r.nsys, self.N)) if r.x is None else r.x
            n, g, xx, v = self.rows_of(self._rows(r), x, r.refine)
            t = np.array(r.t, dtype=float)
            out[r.name] = (t, n, g, xx, v) if per_system else (t, n[:, 0], g[:, 0], xx[:, 0], v[:, 0])
        return out
