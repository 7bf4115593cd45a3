"""Device statistics: per-node statistics over time of model expressions, computed where the state lives.

A statistic is a named expression in the model's own string language (what a probe accepts:
``observers.discretise``), a kind -- ``"mean"``, ``"var"`` (the population variance, ``np.var``'s
default), ``"max"``, ``"min"`` (NaN as NumPy has it), ``"argmax"``, ``"argmin"`` (the ``t`` of the first
sample that attained the extremum) -- and a stride in steps ``every``.  Its samples are the state it was
added at and the state after every ``every``-th step; every sample has the same weight.  The expressions
are lowered by ``codegen.lower_statistics`` and compiled into one more code object of the model
(``observers.py``: what the statistics share with the probes and the recorders); ``tfk_stat``
(``csrc/tf_stat.h``) reads a resident state slot and folds it into the statistic's accumulator planes in
device memory (``tf_stat_*``), which come to the host when the statistic is read.  The sample count
lives here, on the host.  ``nodes`` selects the nodes that are returned; every node is accumulated.

:class:`StatisticSet` is what ``Simulation.add_statistic`` and ``Ensemble.add_statistic`` build on.
"""

import numpy as np

from . import codegen
from .observers import ItemObserverSet, checked_every, checked_nodes, discretise
from .observers import _Bound  # noqa: F401  (the tests build one)

__all__ = ["StatisticSet", "STATISTIC_KINDS", "MAX_STATISTICS"]

#: kinds of a device statistic, in the order of the TF_STAT_* kinds of csrc/tf_args.h
STATISTIC_KINDS = ("mean", "var", "max", "min", "argmax", "argmin")
#: statistics of one set (tf_stat_create)
MAX_STATISTICS = 64


class _Statistic:
    def __init__(self, name, expression, disc, kind, every, window):
        self.name, self.expression, self.disc, self.kind, self.every = name, expression, disc, kind, every
        self.start, self.stop, self.step = window
        self.ncols = -(-(self.stop - self.start) // self.step)
        self.origin = None           # key of the state of sample 1
        self.last = None             # key of the state of the last sample
        self.n = 0                   # samples folded so far
        self.where = None            # the _Bound whose handle holds the accumulators ...
        self.held = None             # ... or they are here, [planes][nsys][N] (no handle holds them)
        self.x = None                # [ncols] or [nsys][ncols]
        self.nsys = 1


class StatisticSet(ItemObserverSet):
    """The statistics of one Simulation or Ensemble (``N`` nodes per system) and their accumulators.

    Samples are folded on the device (``record``) and the accumulators are fetched when the statistics
    are read (``series``): one ``tf_stat`` handle per solver the set has run on, one code object per
    parameter layout / sweep segment of those solvers.  A set that goes on on another solver of the same
    grid takes its accumulators along."""

    kind = "stat"
    _laid_out = "the statistics were laid out for"

    # ---- the set ---------------------------------------------------------------------
    def add(self, name, expression, stat="mean", every=1, nodes=slice(None)):
        """Validate, lower and append one statistic (nothing is computed yet)."""
        if stat not in STATISTIC_KINDS:
            raise ValueError("unknown kind of statistic stat=%r (one of %s)" % (stat, ", ".join(STATISTIC_KINDS)))
        if name in self.names:
            raise ValueError("a statistic named %r exists already" % (name,))
        every = checked_every("statistic", name, every)
        window = checked_nodes("statistic", name, nodes, self.N)
        if len(self._items) >= MAX_STATISTICS:
            raise ValueError("at most %d statistics per simulation" % MAX_STATISTICS)
        disc = discretise(self.model, expression)
        codegen.lower_statistics(self.model, [disc])       # (what the C emitter refuses, refused now)
        self._flush()
        self._items.append(_Statistic(name, expression, disc, stat, every, window))
        self._reset()

    def reset(self, name):
        """Forget the samples of statistic ``name``: the next state that is due is sample 1 again (the
        state of the last sample is not taken a second time).  Nothing happens on the device: sample 1
        overwrites the accumulators."""
        r = self._get(name)
        r.n, r.origin, r.where, r.held = 0, None, None, None

    # ---- device side -----------------------------------------------------------------
    def _lower(self, mask):
        return codegen.lower_statistics(self.model, self.expressions(), parvec_mask=mask)

    def _make_handle(self, solver, code, spec):
        from ._capi import DeviceStat
        exprs = self.expressions()
        geometry = [(exprs.index(r.disc), STATISTIC_KINDS.index(r.kind)) for r in self._items]
        return DeviceStat(solver, code, geometry, len(spec["host_consts"]))

    def record(self, solver, slot, t, key, x, member_pars):
        """Fold state ``slot`` of ``solver`` (a ``DeviceSolver``) into every statistic that is due.
        ``key`` counts the steps (a statistic is due at its first state and every ``every`` keys after
        it, once per key); ``x``: ``[N]`` or ``[nsys][N]``; ``member_pars``: per system, the model's
        parameter values (the host constants of the expressions are computed from them).  A statistic
        that is not due costs nothing on the device.  Accumulators that another solver's handle holds
        (the front end changed its solver), or that came to the host when the set changed, are loaded
        into this solver's handle first: no sample is lost."""
        due = self.due(key)
        if not due:
            return
        x = np.asarray(x, dtype=float)
        b = self._bind_inputs(solver, x, member_pars)
        for k in due:
            r = self._items[k]
            if r.n and r.where is not b:
                if r.where is not None:
                    r.held = r.where.handle.fetch(k)
                b.handle.load(k, r.held)
                r.held = None
            r.where = b
            b.handle.update(k, slot, r.n + 1, t)
            r.n += 1
            if r.origin is None:
                r.origin = key
                r.x = np.array(x[..., r.start:r.stop:r.step])
            r.last, r.nsys = key, solver.nsys

    def _flush(self):
        """The accumulators still on a device to the host (the handles are about to be closed)."""
        for k, r in enumerate(self._items):
            if r.where is not None:
                r.held = r.where.handle.fetch(k) if r.n else None
                r.where = None

    def series(self, per_system=True):
        """name -> (n, x [ncols] or [nsys, ncols], values [nsys, ncols]) (``per_system=False``: x
        [ncols], values [ncols]); ``n``: samples folded so far (0: the values are NaN; ``x`` is the grid
        of the first sample ever taken, None before it)."""
        out = {}
        for k, r in enumerate(self._items):
            if r.n == 0:
                v = np.full((r.nsys, self.N), np.nan)
            else:
                planes = r.where.handle.fetch(k) if r.where is not None else r.held
                if r.kind == "var":
                    v = planes[1] / float(r.n)
                else:
                    v = planes[1] if r.kind in ("argmax", "argmin") else planes[0]
            v = np.array(v[:, r.start:r.stop:r.step])
            x = r.x                              # (None: no sample was ever taken, the grid is not known)
            if x is not None and x.ndim == 2 and (not per_system or (x == x[0]).all()):
                x = x[0]
            out[r.name] = (r.n, x, v if per_system else v[0])
        return out
