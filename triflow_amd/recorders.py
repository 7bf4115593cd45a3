"""Device recorders: decimated space-time series of model expressions, computed where the state lives.

A recorder is a named expression in the model's own string language (what a probe accepts:
``observers.discretise``), a window of nodes ``nodes = slice(start, stop, step)``, a pool over the nodes
of each bin of ``step`` nodes -- ``"sample"`` (the bin's first node), ``"max"``, ``"min"`` (NaN as
NumPy has it), ``"mean"`` (a sum in a fixed order over the bin's node count) -- and a stride in steps
``every``.  Column ``j`` covers nodes ``start + j*step ... min(start + (j+1)*step, stop) - 1`` and
``x[j]`` is the coordinate of the first of them.  The expressions are lowered by
``codegen.lower_records`` and compiled into one more code object of the model (``observers.py``: what the recorders share
with the probes); ``tfk_record``
(``csrc/tf_record.h``) reads a resident state slot and writes one row per record into the recorder's
ring in device memory, which comes to the host half by half on a stream of its own (``tf_record_*``).
A picture of a million nodes leaves the GPU as some KB per recorded row.

:class:`RecorderSet` is what ``Simulation.add_recorder`` and ``Ensemble.add_recorder`` build on.
"""

import numpy as np

from . import codegen
from .codegen import RECORD_POOLS
from .observers import RowItem, RowObserverSet, _is_int, checked_every, checked_nodes, discretise
from .observers import _Bound  # noqa: F401  (the tests build one)

__all__ = ["RecorderSet", "RECORD_POOLS", "DEFAULT_RING_BYTES", "MAX_RING_ROWS", "MAX_RECORDERS"]

#: device ring of one recorder, both halves together (and as much page-locked host memory)
DEFAULT_RING_BYTES = 32 << 20
#: ... but no more rows than this: a run waits for a copy once per half
MAX_RING_ROWS = 2048
#: recorders of one set (tf_record_create)
MAX_RECORDERS = 64


class _Recorder(RowItem):
    def __init__(self, name, expression, disc, every, window, pool, capacity):
        super().__init__(name, expression, disc, every)    # (a row: [nsys][ncols])
        self.pool, self.capacity = pool, capacity
        self.start, self.stop, self.step = window
        self.ncols = -(-(self.stop - self.start) // self.step)
        self.x = None                # [ncols] or [nsys][ncols]

    def rows_of_ring(self, nsys):
        """Rows of the device ring (both halves) on a solver of ``nsys`` systems."""
        if self.capacity is not None:
            return self.capacity
        row = 8 * nsys * self.ncols
        if 2 * row > DEFAULT_RING_BYTES:
            raise ValueError("recorder %r: one row is %d bytes (%d systems x %d columns) and does not fit a "
                             "half of the %d-byte ring: record fewer columns (a larger step of `nodes`)"
                             % (self.name, row, nsys, self.ncols, DEFAULT_RING_BYTES))
        return max(2, min(DEFAULT_RING_BYTES // row, MAX_RING_ROWS) & ~1)


class RecorderSet(RowObserverSet):
    """The recorders of one Simulation or Ensemble (``N`` nodes per system) and their series.

    Rows are recorded on the device (``record``) and fetched when the series are read (``series``):
    one ``tf_record`` handle per solver the set has run on, one code object per parameter layout /
    sweep segment of those solvers.  ``capacity``: rows of every recorder's device ring (default:
    ``DEFAULT_RING_BYTES`` worth of rows)."""

    kind = "record"
    _laid_out = "the recorders were laid out for"

    def __init__(self, model, N, capacity=None):
        super().__init__(model, N)
        self.capacity = capacity

    # ---- the set ---------------------------------------------------------------------
    def add(self, name, expression, every=1, nodes=slice(None), pool="sample", capacity=None):
        """Validate, lower and append one recorder (nothing is computed yet)."""
        if pool not in RECORD_POOLS:
            raise ValueError("unknown recorder pool %r (one of %s)" % (pool, ", ".join(RECORD_POOLS)))
        if name in self.names:
            raise ValueError("a recorder named %r exists already" % (name,))
        every = checked_every("recorder", name, every)
        window = checked_nodes("recorder", name, nodes, self.N)
        capacity = self.capacity if capacity is None else capacity
        if capacity is not None and (not _is_int(capacity) or capacity < 2):
            raise ValueError("recorder %r: capacity=%r, the ring has two rows at least (one per half)"
                             % (name, capacity))
        if len(self._items) >= MAX_RECORDERS:
            raise ValueError("at most %d recorders per simulation" % MAX_RECORDERS)
        disc = discretise(self.model, expression)
        codegen.lower_records(self.model, [disc])          # (what the C emitter refuses, refused now)
        self._flush()
        self._items.append(_Recorder(name, expression, disc, every, window, pool,
                                     None if capacity is None else int(capacity) & ~1))
        self._reset()

    # ---- device side -----------------------------------------------------------------
    def _lower(self, mask):
        return codegen.lower_records(self.model, self.expressions(), parvec_mask=mask)

    def _make_handle(self, solver, code, spec):
        from ._capi import DeviceRecord
        exprs = self.expressions()
        geometry = [(exprs.index(r.disc), RECORD_POOLS.index(r.pool), r.start, r.stop, r.step, r.rows_of_ring(solver.nsys))
                    for r in self._items]
        return DeviceRecord(solver, code, geometry, len(spec["host_consts"]))

    def _first_row(self, r, x, solver):
        r.x = np.array(x[..., r.start:r.stop:r.step])

    def _no_rows(self, r):
        return np.zeros((0, r.nsys, r.ncols))

    def series(self, per_system=True):
        """name -> (t [rows], x [ncols] or [nsys, ncols], values [rows, nsys, ncols])
        (``per_system=False``: x [ncols], values [rows, ncols])."""
        self._flush()
        out = {}
        for r in self._items:
            v = self._rows(r)
            x = np.zeros(r.ncols) if r.x is None else r.x
            if x.ndim == 2 and (not per_system or (x == x[0]).all()):
                x = x[0]
            out[r.name] = (np.array(r.t, dtype=float), x, v if per_system else v[:, 0])
        return out

    def save(self, name, path, metadata=None):
        """Recorder ``name`` of a single system as a container directory (``container.write_series``)."""
        from .container import write_series
        self._get(name)
        t, x, values = self.series(per_system=False)[name]
        return write_series(path, t, x, {name: values}, metadata or {})
