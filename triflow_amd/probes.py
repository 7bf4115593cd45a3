"""Device probes: per-step reductions of model expressions, computed where the state lives.

A probe is a named expression in the model's own string language (dependent variables, help
functions, parameters, ``x``, ``dxU``, ``dx(...)``, ``upwind(...)``) and a reduction over the nodes
of each system: ``sum``, ``mean``, ``integral`` (``np.trapz`` with the model's spacing; ``dx * sum``
on a periodic grid), ``max``, ``min``, ``argmax``, ``argmin`` (the coordinate ``x`` of the first node
at the extremum).  The expression is discretised with the model's stencils (on a copy: the model
is not touched), lowered by ``codegen.lower_probes`` and compiled into a second code object of the
model (``observers.py``: what the probes share with the recorders); the probe kernels
(``csrc/tf_probe.h``) read a resident state slot and write one row per
record into a ring in device memory, which comes to the host in batches (``tf_probe_*``).

:class:`ProbeSet` is what ``Simulation.add_probe`` and ``Ensemble.add_probe`` build on.
"""

import numpy as np

from . import codegen
from .codegen import PROBE_REDUCTIONS
from .observers import ObserverSet, discretise

__all__ = ["ProbeSet", "discretise", "PROBE_REDUCTIONS", "DEFAULT_CAPACITY", "MAX_PROBES"]

#: rows of the device ring: a run waits for the GPU once per this many records
DEFAULT_CAPACITY = 1024
#: probes of one set (tf_probe_create)
MAX_PROBES = 64


class ProbeSet(ObserverSet):
    """The probes of one Simulation or Ensemble and their recorded series.

    Rows are recorded on the device (``record``) and fetched when the series are read
    (``series``): one ``tf_probe`` handle per solver the set has run on, one code object per
    parameter layout / sweep segment of those solvers."""

    kind = "probe"

    def __init__(self, model, capacity=None):
        super().__init__(model)
        self.capacity = int(capacity or DEFAULT_CAPACITY)
        self._probes = []            # [(name, expression, reduction, discretised expression)]
        self._series = {}            # name -> ([t], [values [nsys]], key of the last row)
        self._pending = []           # rows on the device, in record order: (_Bound, t, key)
        self._nsys = 1               # systems of the solver last recorded on

    # ---- the set ---------------------------------------------------------------------
    @property
    def names(self):
        return [p[0] for p in self._probes]

    def add(self, name, expression, reduce="sum"):
        """Validate, lower and append one probe (nothing is computed yet)."""
        if reduce not in PROBE_REDUCTIONS:
            raise ValueError("unknown probe reduction %r (one of %s)" % (reduce, ", ".join(PROBE_REDUCTIONS)))
        if name in self.names:
            raise ValueError("a probe named %r exists already" % (name,))
        if len(self._probes) >= MAX_PROBES:
            raise ValueError("at most %d probes per simulation" % MAX_PROBES)
        disc = discretise(self.model, expression)
        codegen.lower_probes(self.model, [disc], [reduce])      # (what the C emitter refuses, refused now)
        self._flush()
        self._probes.append((name, expression, reduce, disc))
        self._series[name] = ([], [], None)
        self._reset()

    def remove(self, name):
        if name not in self.names:
            raise KeyError(name)
        self._flush()
        self._probes = [p for p in self._probes if p[0] != name]
        del self._series[name]
        self._reset()

    # ---- device side -----------------------------------------------------------------
    def _lower(self, mask):
        return codegen.lower_probes(self.model, [p[3] for p in self._probes], [p[2] for p in self._probes],
                                    parvec_mask=mask)

    def _make_handle(self, solver, code, spec):
        from ._capi import DeviceProbe
        return DeviceProbe(solver, code, spec["kinds"], len(spec["host_consts"]), self.capacity)

    def record(self, solver, slot, t, key, x, member_pars):
        """Queue one row: the probes of state ``slot`` of ``solver`` (a ``DeviceSolver``).  ``key``
        names the state (a probe that already has a row for it gets none: ``add`` records the
        current state for the new probe only); ``x``: ``[N]`` or ``[nsys][N]``; ``member_pars``: per
        system, the model's parameter values (the probes' host constants are computed from them)."""
        if not self._probes:
            return
        b = self._bind_inputs(solver, np.asarray(x, dtype=float), member_pars)
        b.handle.record(slot)
        self._pending.append((b, t, key))
        self._nsys = solver.nsys

    def _flush(self):
        """Fetch every row still on the device and append it to the series."""
        if not self._pending:
            return
        rows = {}
        for b, _, _ in self._pending:
            if id(b) not in rows:
                rows[id(b)] = iter(b.handle.fetch())
        for b, t, key in self._pending:
            row = next(rows[id(b)])                      # [nsys][nprobe]
            for k, p in enumerate(self._probes):
                ts, vals, last = self._series[p[0]]
                if last is not None and last == key:
                    continue
                ts.append(t)
                vals.append(row[:, k].copy())
                self._series[p[0]] = (ts, vals, key)
        self._pending.clear()

    def series(self, per_system=True):
        """name -> (t [rows], values [rows, nsys]) (``per_system=False``: values [rows])."""
        self._flush()
        out = {}
        for p in self._probes:
            ts, vals, _ = self._series[p[0]]
            v = np.array(vals, dtype=float).reshape(len(vals), self._nsys)
            out[p[0]] = (np.array(ts, dtype=float), v if per_system else v[:, 0])
        return out
