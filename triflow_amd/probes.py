"""Device probes: per-step reductions of model expressions, computed where the state lives.

A probe is a named expression in the model's own string language (dependent variables, help
functions, parameters, ``x``, ``dxU``, ``dx(...)``, ``upwind(...)``) and a reduction over the nodes
of each system: ``sum``, ``mean``, ``integral`` (``np.trapz`` with the model's spacing; ``dx * sum``
on a periodic grid), ``max``, ``min``, ``argmax``, ``argmin`` (the coordinate ``x`` of the first node
at the extremum).  The expression is discretised with the model's stencils (on a copy: the model
is not touched), lowered by ``codegen.lower_probes`` and compiled into a second code object of the
model; the probe kernels (``csrc/tf_probe.h``) read a resident state slot and write one row per
record into a ring in device memory, which comes to the host in batches (``tf_probe_*``).

:class:`ProbeSet` is what ``Simulation.add_probe`` and ``Ensemble.add_probe`` build on.
"""

import numpy as np
import sympy as sp
from sympy.core.function import AppliedUndef

from . import codegen
from .codegen import PROBE_REDUCTIONS, UnsupportedExpression

__all__ = ["ProbeSet", "discretise", "PROBE_REDUCTIONS", "DEFAULT_CAPACITY", "MAX_PROBES"]

#: rows of the device ring: a run waits for the GPU once per this many records
DEFAULT_CAPACITY = 1024
#: probes of one set (tf_probe_create)
MAX_PROBES = 64


def discretise(model, expression):
    """Probe string -> SymPy expression over ``model._symbolic_args``, discretised with the model's
    stencils (``Model._discretise`` on a copy: the model's footprint, bounds and code object stay
    what they are).  Raises ``ValueError`` for what the model's parser refuses and for unknown
    symbols, :class:`UnsupportedExpression` for a stencil wider than the model's window."""
    if not isinstance(expression, str):
        raise ValueError("badly formated probe expression %r: a string is expected" % (expression,))
    (expr,) = model._parse_strings((expression,))
    work = object.__new__(type(model))
    work.__dict__.update(model.__dict__)
    before = {k: set(v) for k, v in model._symb_vars_with_spatial_diff_order.items()}
    work._symb_vars_with_spatial_diff_order = {k: set(v) for k, v in before.items()}
    try:
        (disc,) = work._discretise((expr,))
    except NotImplementedError as exc:
        raise UnsupportedExpression("probe %r: %s" % (expression, exc))
    limit = (model._window_range - 1) // 2
    for name, touched in work._symb_vars_with_spatial_diff_order.items():
        for _, off in touched - before[name]:
            if abs(off) > limit:
                raise UnsupportedExpression(
                    "probe %r reads %s at node offset %+d: a probe reads the model's own stencil window, "
                    "of half width %d here (offsets -%d ... +%d)" % (expression, name, off, limit, limit, limit))
    allowed = set(model._symbolic_args)
    unknown = sorted(str(s) for s in disc.free_symbols - allowed)
    undefined = sorted(str(f.func) for f in disc.atoms(AppliedUndef))
    if unknown or undefined:
        raise ValueError("badly formated probe expression %r: unknown %s"
                         % (expression, ", ".join(unknown + [f + "(...)" for f in undefined])))
    return sp.sympify(disc)


class _Bound:
    """One ``tf_probe`` (the probe kernels on one solver) and what was last uploaded to it."""

    def __init__(self, handle, spec):
        self.handle, self.spec, self.key = handle, spec, None


class ProbeSet:
    """The probes of one Simulation or Ensemble and their recorded series.

    Rows are recorded on the device (``record``) and fetched when the series are read
    (``series``): one ``tf_probe`` handle per solver the set has run on, one code object per
    parameter layout / sweep segment of those solvers."""

    def __init__(self, model, capacity=None):
        self.model = model
        self.capacity = int(capacity or DEFAULT_CAPACITY)
        self._probes = []            # [(name, expression, reduction, discretised expression)]
        self._series = {}            # name -> ([t], [values [nsys]], key of the last row)
        self._bound = {}             # id(solver) -> _Bound
        self._blocks = {}            # parvec mask -> (probe block, spec)
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

    def _reset(self):
        for b in self._bound.values():
            b.handle.close()
        self._bound.clear()
        self._blocks.clear()

    def close(self):
        self._flush()
        self._reset()

    # ---- device side -----------------------------------------------------------------
    def _lowered(self, mask):
        if mask not in self._blocks:
            self._blocks[mask] = codegen.lower_probes(self.model, [p[3] for p in self._probes],
                                                      [p[2] for p in self._probes], parvec_mask=mask)
        return self._blocks[mask]

    def _bind(self, solver):
        b = self._bound.get(id(solver))
        if b is not None and b.handle.solver is solver:
            return b
        from . import compilers
        from ._capi import DeviceProbe
        spec = solver.model.spec
        block, pspec = self._lowered(spec["parvec_mask"])
        hsaco = compilers.build_probe_code_object(self.model, block, spec["parvec_mask"], spec["seg"],
                                                  spec["sweep_block"])
        with open(hsaco, "rb") as f:
            code = f.read()
        handle = DeviceProbe(solver, code, pspec["kinds"], len(pspec["host_consts"]), self.capacity)
        b = self._bound[id(solver)] = _Bound(handle, pspec)
        return b

    def record(self, solver, slot, t, key, x, member_pars):
        """Queue one row: the probes of state ``slot`` of ``solver`` (a ``DeviceSolver``).  ``key``
        names the state (a probe that already has a row for it gets none: ``add`` records the
        current state for the new probe only); ``x``: ``[N]`` or ``[nsys][N]``; ``member_pars``: per
        system, the model's parameter values (the probes' host constants are computed from them)."""
        if not self._probes:
            return
        b = self._bind(solver)
        x = np.asarray(x, dtype=float)
        bkey = (x.shape, float(x.flat[0]), float(x.flat[-1]),
                tuple(tuple(float(np.ravel(v)[0]) for v in pars) for pars in member_pars))
        if bkey != b.key:
            x2 = np.broadcast_to(x, (solver.nsys, solver.N))
            if not solver.model.spec["uses_x"]:          # (else the probes read the solver's own x plane)
                b.handle.set_x(x2)
            if b.spec["host_consts"]:
                dxs = (x2[:, -1] - x2[:, 0]) / (solver.N - 1)
                b.handle.set_consts(np.array([codegen.eval_host_constants(b.spec, dxs[e], member_pars[e])
                                              for e in range(solver.nsys)]))
            b.key = bkey
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
