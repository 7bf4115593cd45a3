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
from .observers import ObserverSet, _Bound, discretise  # noqa: F401  (_Bound: the tests build one)

__all__ = ["RecorderSet", "RECORD_POOLS", "DEFAULT_RING_BYTES", "MAX_RING_ROWS", "MAX_RECORDERS"]

#: device ring of one recorder, both halves together (and as much page-locked host memory)
DEFAULT_RING_BYTES = 32 << 20
#: ... but no more rows than this: a run waits for a copy once per half
MAX_RING_ROWS = 2048
#: recorders of one set (tf_record_create)
MAX_RECORDERS = 64


class _Recorder:
    def __init__(self, name, expression, disc, every, window, pool, capacity):
        self.name, self.expression, self.disc = name, expression, disc
        self.every, self.pool, self.capacity = every, pool, capacity
        self.start, self.stop, self.step = window
        self.ncols = -(-(self.stop - self.start) // self.step)
        self.origin = None           # key of the state of the first row
        self.last = None             # key of the state of the last row
        self.pending = []            # rows on the device, in record order: (_Bound, t)
        self.t, self.blocks = [], []   # fetched: t per row, arrays [rows][nsys][ncols] in record order
        self.x = None                # [ncols] or [nsys][ncols]
        self.nsys = 1

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


class RecorderSet(ObserverSet):
    """The recorders of one Simulation or Ensemble (``N`` nodes per system) and their series.

    Rows are recorded on the device (``record``) and fetched when the series are read (``series``):
    one ``tf_record`` handle per solver the set has run on, one code object per parameter layout /
    sweep segment of those solvers.  ``capacity``: rows of every recorder's device ring (default:
    ``DEFAULT_RING_BYTES`` worth of rows)."""

    kind = "record"

    def __init__(self, model, N, capacity=None):
        super().__init__(model)
        self.N = int(N)
        self.capacity = capacity
        self._recs = []

    # ---- the set ---------------------------------------------------------------------
    @property
    def names(self):
        return [r.name for r in self._recs]

    def _get(self, name):
        for r in self._recs:
            if r.name == name:
                return r
        raise KeyError(name)

    def add(self, name, expression, every=1, nodes=slice(None), pool="sample", capacity=None):
        """Validate, lower and append one recorder (nothing is computed yet)."""
        if pool not in RECORD_POOLS:
            raise ValueError("unknown recorder pool %r (one of %s)" % (pool, ", ".join(RECORD_POOLS)))
        if name in self.names:
            raise ValueError("a recorder named %r exists already" % (name,))
        if isinstance(every, bool) or not isinstance(every, (int, np.integer)) or every < 1:
            raise ValueError("recorder %r: every=%r, an integer >= 1 is expected" % (name, every))
        if not isinstance(nodes, slice):
            raise ValueError("recorder %r: nodes=%r, a slice is expected" % (name, nodes))
        try:
            window = nodes.indices(self.N)
        except (TypeError, ValueError) as exc:
            raise ValueError("recorder %r: nodes=%r: %s" % (name, nodes, exc))
        if window[2] < 1:
            raise ValueError("recorder %r: nodes=%r, a step >= 1 is expected" % (name, nodes))
        if window[1] <= window[0]:
            raise ValueError("recorder %r: nodes=%r holds no node of a grid of %d" % (name, nodes, self.N))
        capacity = self.capacity if capacity is None else capacity
        if capacity is not None and (isinstance(capacity, bool) or not isinstance(capacity, (int, np.integer))
                                     or capacity < 2):
            raise ValueError("recorder %r: capacity=%r, the ring has two rows at least (one per half)"
                             % (name, capacity))
        if len(self._recs) >= MAX_RECORDERS:
            raise ValueError("at most %d recorders per simulation" % MAX_RECORDERS)
        disc = discretise(self.model, expression)
        codegen.lower_records(self.model, [disc])          # (what the C emitter refuses, refused now)
        self._flush()
        self._recs.append(_Recorder(name, expression, disc, int(every), window, pool,
                                    None if capacity is None else int(capacity) & ~1))
        self._reset()

    def remove(self, name):
        self._get(name)
        self._flush()
        self._recs = [r for r in self._recs if r.name != name]
        self._reset()

    # ---- device side -----------------------------------------------------------------
    def expressions(self):
        """The distinct discretised expressions of the set, in the order they were added: recorders
        of one expression share a case of the record block (and sets that differ only in geometry
        share a code object)."""
        out = []
        for r in self._recs:
            if r.disc not in out:
                out.append(r.disc)
        return out

    def _lower(self, mask):
        return codegen.lower_records(self.model, self.expressions(), parvec_mask=mask)

    def _bind(self, solver):
        if solver.N != self.N:
            raise ValueError("the recorders were laid out for %d nodes, the solver has %d" % (self.N, solver.N))
        return super()._bind(solver)

    def _make_handle(self, solver, code, spec):
        from ._capi import DeviceRecord
        exprs = self.expressions()
        geometry = [(exprs.index(r.disc), RECORD_POOLS.index(r.pool), r.start, r.stop, r.step, r.rows_of_ring(solver.nsys))
                    for r in self._recs]
        return DeviceRecord(solver, code, geometry, len(spec["host_consts"]))

    def record(self, solver, slot, t, key, x, member_pars):
        """Queue a row of every recorder that is due: state ``slot`` of ``solver`` (a ``DeviceSolver``).
        ``key`` counts the steps (a recorder is due at its first state and every ``every`` keys after
        it, once per key); ``x``: ``[N]`` or ``[nsys][N]``; ``member_pars``: per system, the model's
        parameter values (the host constants of the expressions are computed from them).  A recorder
        that is not due costs nothing on the device."""
        due = [k for k, r in enumerate(self._recs)
               if r.last != key and (r.origin is None or (key - r.origin) % r.every == 0)]
        if not due:
            return
        x = np.asarray(x, dtype=float)
        b = self._bind_inputs(solver, x, member_pars)
        for k in due:
            r = self._recs[k]
            b.handle.record(k, slot)
            r.pending.append((b, t))
            if r.origin is None:
                r.origin = key
                r.x = np.array(x[..., r.start:r.stop:r.step])
            r.last, r.nsys = key, solver.nsys

    def _flush(self):
        """Fetch every row still on the device and append it to the series (whole blocks: the rows of
        a long run are copied once here and once when the blocks are joined)."""
        for k, r in enumerate(self._recs):
            if not r.pending:
                continue
            bounds = []
            for b, _ in r.pending:
                if not any(b is o for o in bounds):
                    bounds.append(b)
            fetched = {id(b): b.handle.fetch(k) for b in bounds}
            if len(bounds) == 1:
                r.blocks.append(fetched[id(bounds[0])])
            else:                                        # (several solvers in turn: row by row, in record order)
                at = {id(b): 0 for b in bounds}
                for b, _ in r.pending:
                    r.blocks.append(fetched[id(b)][at[id(b)]:at[id(b)] + 1])
                    at[id(b)] += 1
            r.t.extend(t for _, t in r.pending)
            r.pending.clear()

    def series(self, per_system=True):
        """name -> (t [rows], x [ncols] or [nsys, ncols], values [rows, nsys, ncols])
        (``per_system=False``: x [ncols], values [rows, ncols])."""
        self._flush()
        out = {}
        for r in self._recs:
            if len(r.blocks) != 1:
                r.blocks = [np.concatenate(r.blocks) if r.blocks else np.zeros((0, r.nsys, r.ncols))]
            v = r.blocks[0]
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
