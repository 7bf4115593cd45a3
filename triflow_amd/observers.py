"""Device observers: what the probes (``probes.py``), the recorders (``recorders.py``), the statistics
(``statistics.py``), the spectra (``spectra.py``), the extrema (``extrema.py``) and the histograms
(``histograms.py``) share.

An observer evaluates expressions in the model's own string language at the nodes of a resident state
slot.  All kinds go through the same node core (``csrc/tf_node.h``): the expressions are discretised with
the model's stencils (``discretise``), lowered to a block of C that follows the model's generated body,
and compiled with the header of their kind into one more code object of the model, which holds that kind's
kernels alone (``compilers.build_observer_code_object``); a handle per solver binds it (``_capi.DeviceProbe`` ...) and is fed ``x`` and the host constants of the
expressions.  :class:`ObserverSet` owns that part.

:class:`ItemObserverSet` adds what the sets of named items with a stride share (all kinds but the probes):
the item list, the distinct expressions, the due rule, the check of the solver's grid, and the validators
of ``every``, ``nodes`` and ``capacity`` (``checked_*``).  :class:`RowObserverSet` adds the series of the
kinds that write one row per record into a ring per item (recorders, spectra, extrema, histograms):
``record``, the fetch of the rows still on the device (``_flush``) and their joining.  A kind supplies its
item, the specific parts of ``add``, the lowering of its expressions, its handle and what a row is.
:class:`Observed` is the ``add_*`` / ``remove_*`` side of the front ends.
"""

import importlib

import numpy as np
import sympy as sp
from sympy.core.function import AppliedUndef

from . import codegen
from .codegen import UnsupportedExpression

__all__ = ["ObserverSet", "ItemObserverSet", "RowObserverSet", "Observed", "discretise"]


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
    """One handle (the observer's kernels on one solver) and what was last uploaded to it."""

    def __init__(self, handle, spec):
        self.handle, self.spec, self.key = handle, spec, None


class ObserverSet:
    """The code objects and handles of a set of observers: one handle per solver the set has run on, one
    code object per parameter layout / sweep segment of those solvers.  Subclasses: ``kind`` ("probe" /
    "record" / "stat" / "spectrum" / "extrema" / "histogram": ``compilers.build_observer_code_object``),
    ``_lower(mask) -> (block, spec)``, ``_make_handle(solver, code, spec)`` and ``_flush()`` (everything
    still on the device to the host)."""

    kind = None

    def __init__(self, model):
        self.model = model
        self._bound = {}             # id(solver) -> _Bound
        self._blocks = {}            # parvec mask -> (block, spec)

    def _reset(self):
        for b in self._bound.values():
            b.handle.close()
        self._bound.clear()
        self._blocks.clear()

    def close(self):
        self._flush()
        self._reset()

    def _lowered(self, mask):
        if mask not in self._blocks:
            self._blocks[mask] = self._lower(mask)
        return self._blocks[mask]

    def _bind(self, solver):
        b = self._bound.get(id(solver))
        if b is not None and b.handle.solver is solver:
            return b
        from . import compilers
        spec = solver.model.spec
        block, ospec = self._lowered(spec["parvec_mask"])
        hsaco = compilers.build_observer_code_object(self.model, block, self.kind, spec["parvec_mask"],
                                                     spec["seg"], spec["sweep_block"])
        with open(hsaco, "rb") as f:
            code = f.read()
        b = self._bound[id(solver)] = _Bound(self._make_handle(solver, code, ospec), ospec)
        return b

    def _bind_inputs(self, solver, x, member_pars):
        """The set's binding to ``solver``, its inputs up to date: ``x`` (``[N]`` or ``[nsys][N]``) and
        the host constants of the expressions, computed from ``member_pars`` (per system, the model's
        parameter values), are uploaded when they changed since the last record."""
        b = self._bind(solver)
        bkey = (x.shape, float(x.flat[0]), float(x.flat[-1]),
                tuple(tuple(float(np.ravel(v)[0]) for v in pars) for pars in member_pars))
        if bkey != b.key:
            x2 = np.broadcast_to(x, (solver.nsys, solver.N))
            if not solver.model.spec["uses_x"]:          # (else the kernels read the solver's own x plane)
                b.handle.set_x(x2)
            if b.spec["host_consts"]:
                dxs = (x2[:, -1] - x2[:, 0]) / (solver.N - 1)
                b.handle.set_consts(np.array([codegen.eval_host_constants(b.spec, dxs[e], member_pars[e])
                                              for e in range(solver.nsys)]))
            b.key = bkey
        return b


def _is_int(v):
    """An integer, and not a bool (Python's or NumPy's)."""
    return not isinstance(v, (bool, np.bool_)) and isinstance(v, (int, np.integer))


def checked_every(noun, name, every):
    """``every`` of ``add`` as an int, or ``ValueError`` (``noun``: "recorder", "spectrum" ...)."""
    if not _is_int(every) or every < 1:
        raise ValueError("%s %r: every=%r, an integer >= 1 is expected" % (noun, name, every))
    return int(every)


def checked_nodes(noun, name, nodes, N):
    """``nodes`` of ``add`` as ``slice.indices(N)`` with a step >= 1 and a node at least, or ``ValueError``."""
    if not isinstance(nodes, slice):
        raise ValueError("%s %r: nodes=%r, a slice is expected" % (noun, name, nodes))
    try:
        window = nodes.indices(N)
    except (TypeError, ValueError) as exc:
        raise ValueError("%s %r: nodes=%r: %s" % (noun, name, nodes, exc))
    if window[2] < 1:
        raise ValueError("%s %r: nodes=%r, a step >= 1 is expected" % (noun, name, nodes))
    if window[1] <= window[0]:
        raise ValueError("%s %r: nodes=%r holds no node of a grid of %d" % (noun, name, nodes, N))
    return window


def checked_capacity(noun, name, capacity):
    """``capacity`` of ``add`` (rows of a ring of one row at least) as an int, None as None, or ``ValueError``."""
    if capacity is None:
        return None
    if not _is_int(capacity) or capacity < 1:
        raise ValueError("%s %r: capacity=%r, the ring has one row at least" % (noun, name, capacity))
    return int(capacity)


class ItemObserverSet(ObserverSet):
    """A set of named items -- each an expression and a stride ``every`` -- laid out for a grid of ``N``
    nodes: what the statistics share with the kinds that record rows.  An item has ``name``, ``disc``,
    ``every``, ``origin`` and ``last`` (the keys of its first and its latest state).  Subclasses:
    ``_laid_out``, the opening of the message for a solver of another grid."""

    _laid_out = None

    def __init__(self, model, N):
        super().__init__(model)
        self.N = int(N)
        self._items = []

    @property
    def names(self):
        return [r.name for r in self._items]

    def _get(self, name):
        for r in self._items:
            if r.name == name:
                return r
        raise KeyError(name)

    def remove(self, name):
        self._get(name)
        self._flush()
        self._items = [r for r in self._items if r.name != name]
        self._reset()

    def expressions(self):
        """The distinct discretised expressions of the set, in the order they were added: items of one
        expression share a case of the generated block, and sets that differ only in what is data of
        the handle or a launch argument share a code object."""
        out = []
        for r in self._items:
            if r.disc not in out:
                out.append(r.disc)
        return out

    def _bind(self, solver):
        if solver.N != self.N:
            raise ValueError("%s %d nodes, the solver has %d" % (self._laid_out, self.N, solver.N))
        return super()._bind(solver)

    def due(self, key):
        """Indices of the items that take the state ``key`` (``key`` counts the steps): an item is due
        at its first state and every ``every`` keys after it, once per key."""
        return [k for k, r in enumerate(self._items)
                if r.last != key and (r.origin is None or (key - r.origin) % r.every == 0)]


class RowItem:
    """What an item of a :class:`RowObserverSet` keeps of its series."""

    def __init__(self, name, expression, disc, every):
        self.name, self.expression, self.disc, self.every = name, expression, disc, every
        self.origin = None           # key of the state of the first row
        self.last = None             # key of the state of the last row
        self.pending = []            # rows on the device, in record order: (_Bound, t)
        self.t, self.blocks = [], []   # fetched: t per row, arrays [rows][nsys][width] in record order
        self.nsys = 1


class RowObserverSet(ItemObserverSet):
    """The kinds that write one row per record into a ring of their item on the device (recorders,
    spectra, extrema, histograms): rows are queued by ``record`` and come to the host, whole rings at a
    time, when the series are read, the set changes or it is closed (``_flush``).  The handle has
    ``record(k, slot)`` and ``fetch(k) -> [rows][nsys][width]``.  Subclasses: ``_first_row`` where an
    item keeps something of the grid, and ``_no_rows``."""

    def record(self, solver, slot, t, key, x, member_pars):
        """Queue a row of every item that is due (``due``): state ``slot`` of ``solver`` (a
        ``DeviceSolver``).  ``x``: ``[N]`` or ``[nsys][N]``; ``member_pars``: per system, the model's
        parameter values (the host constants of the expressions are computed from them).  An item
        that is not due costs nothing on the device."""
        due = self.due(key)
        if not due:
            return
        x = np.asarray(x, dtype=float)
        b = self._bind_inputs(solver, x, member_pars)
        for k in due:
            r = self._items[k]
            b.handle.record(k, slot)
            r.pending.append((b, t))
            if r.origin is None:
                r.origin = key
                self._first_row(r, x, solver)
            r.last, r.nsys = key, solver.nsys

    def _first_row(self, item, x, solver):
        """What ``item`` keeps of the grid ``x`` (``[N]`` or ``[nsys][N]``) of its first row."""

    def _flush(self):
        """Fetch every row still on the device and append it to the series (whole blocks: the rows of
        a long run are copied once here and once when the blocks are joined)."""
        for k, r in enumerate(self._items):
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

    def _rows(self, item):
        """The fetched rows of ``item`` as one array ``[rows][nsys][width]`` (``_no_rows(item)`` when
        there are none), kept as its only block."""
        if len(item.blocks) != 1:
            item.blocks = [np.concatenate(item.blocks) if item.blocks else self._no_rows(item)]
        return item.blocks[0]


class Observed:
    """``add_probe`` / ``add_recorder`` / ``add_statistic`` / ``add_spectrum`` / ``add_extrema`` /
    ``add_histogram`` ... of a front end (``Simulation``, ``Ensemble``): reductions over space, decimated
    space-time pictures, reductions over time, Fourier amplitudes, the crests and troughs and the
    distribution of values over time.  The front end has ``model``, says how a set records its current
    state (``_record_on(series_set)``: it also calls it after every step for each of ``_observer_sets()``),
    how many nodes a system has (``_n_nodes``) and whether its series keep the axis of the systems
    (``_per_system``)."""

    #: the kinds, in the order they record a state: the attribute that holds the set (None until the first
    #: ``add_*``), its module and class, and whether the set is laid out for the number of nodes
    _KINDS = (("_probes", "probes", "ProbeSet", False),
              ("_recorders", "recorders", "RecorderSet", True),
              ("_statistics", "statistics", "StatisticSet", True),
              ("_spectra", "spectra", "SpectrumSet", True),
              ("_extrema", "extrema", "ExtremaSet", True),
              ("_histograms", "histograms", "HistogramSet", True))
    _probes = _recorders = _statistics = _spectra = _extrema = _histograms = None
    _per_system = True

    def _observer_sets(self):
        """The sets that exist, in the order of ``_KINDS``."""
        return [getattr(self, attr) for attr, *_ in self._KINDS if getattr(self, attr) is not None]

    def _add_observer(self, attr, name, *args):
        """``add(name, *args)`` on the set ``attr``, created now if this is its first item, and a row of
        the current state."""
        series_set = getattr(self, attr)
        if series_set is None:
            _, module, cls, takes_n = next(kind for kind in self._KINDS if kind[0] == attr)
            cls = getattr(importlib.import_module("." + module, __package__), cls)
            series_set = cls(self.model, self._n_nodes) if takes_n else cls(self.model)
            setattr(self, attr, series_set)
        series_set.add(name, *args)
        try:
            self._record_on(series_set)
        except Exception:
            # (no code object / no handle for the new set: the new one is not kept, the others go on)
            series_set.remove(name)
            raise

    def _observer_set_of(self, attr, name):
        """The set ``attr`` that should hold ``name``; ``KeyError(name)`` when nothing was ever added to it."""
        if getattr(self, attr) is None:
            raise KeyError(name)
        return getattr(self, attr)

    def _series(self, attr):
        series_set = getattr(self, attr)
        return series_set.series(per_system=self._per_system) if series_set is not None else {}

    # ---- device probes (probes.py) ----------------------------------------------------
    def add_probe(self, name, expression, reduce="sum"):
        """Record ``reduce`` of the model expression ``expression`` over the nodes (of every member of
        an ensemble) after every step, on the GPU (``probes.py``): the t0 row now, then one row after
        every step (a Simulation: where the post-processes run).  The series is ``probes[name] =
        (t, values)``, an Ensemble's ``(t, values[rows, nsys])`` of this rank's members only; the
        fields are never brought to the host for it."""
        self._add_observer("_probes", name, expression, reduce)

    def remove_probe(self, name):
        self._observer_set_of("_probes", name).remove(name)

    @property
    def probes(self):
        """name -> (t, values): float64 arrays, one entry per recorded state."""
        return self._series("_probes")

    # ---- device recorders (recorders.py) ----------------------------------------------
    def add_recorder(self, name, expression, every=1, nodes=slice(None), pool="sample", capacity=None):
        """Record the model expression ``expression`` on the GPU at the columns ``nodes`` (a slice; a
        column is the ``pool`` -- "sample", "max", "min", "mean" -- of a bin of ``nodes.step`` nodes):
        a row now, then after every ``every``-th step (a Simulation: where the post-processes run).
        The series is ``recorders[name] = (t, x, values[rows, ncols])``, an Ensemble's ``(t, x,
        values[rows, nsys, ncols])`` with ``x [nsys, ncols]`` when the members have grids of their own,
        of this rank's members only; the fields never come to the host for it."""
        self._add_observer("_recorders", name, expression, every, nodes, pool, capacity)

    def remove_recorder(self, name):
        self._observer_set_of("_recorders", name).remove(name)

    @property
    def recorders(self):
        """name -> (t, x, values): float64 arrays, one row of values per recorded state."""
        return self._series("_recorders")

    # ---- device statistics (statistics.py) --------------------------------------------
    def add_statistic(self, name, expression, stat="mean", every=1, nodes=slice(None)):
        """Accumulate the statistic ``stat`` -- "mean", "var", "max", "min", "argmax", "argmin" (the
        ``t`` of the first extremal sample) -- over time of the model expression ``expression`` at every
        node, on the GPU (``statistics.py``): the current state is sample 1, then the state after every
        ``every``-th step is a sample (a Simulation: where the post-processes run), all of one weight.
        ``statistics[name] = (n, x, values[ncols])`` at the nodes ``nodes`` (a slice), an Ensemble's
        ``(n, x, values[nsys, ncols])`` of this rank's members only; the fields never come to the host
        for it."""
        self._add_observer("_statistics", name, expression, stat, every, nodes)

    def remove_statistic(self, name):
        self._observer_set_of("_statistics", name).remove(name)

    def reset_statistic(self, name):
        """Drop the samples taken so far (a transient): the next due state is sample 1 again."""
        self._observer_set_of("_statistics", name).reset(name)

    @property
    def statistics(self):
        """name -> (n, x, values): the samples folded so far, float64 arrays over the nodes."""
        return self._series("_statistics")

    # ---- device spectra (spectra.py) ----------------------------------------------------
    def add_spectrum(self, name, expression, modes, every=1, capacity=None):
        """Record the Fourier amplitudes ``c[i] = sum_g v_g * exp(-2j * pi * modes[i] * g / N)`` of the
        model expression ``expression`` (``v`` at the nodes ``g = 0 ... N - 1``) on the GPU
        (``spectra.py``): ``np.fft.fft(v)[modes]``, unnormalised, no window, nothing subtracted (write
        ``h - 1``).  ``periodic=False`` gets the same sum over the node sequence.  ``modes``: up to
        ``spectra.MAX_MODES`` distinct integers in ``0 ... N // 2``.  A row now, then after every
        ``every``-th step (a Simulation: where the post-processes run); ``capacity``: rows of the ring in
        device memory (default 1024).  The series is ``spectra[name] = (t, k, c[rows, nmodes])`` with
        the wavenumbers ``k = 2 * pi * modes / (N * dx)`` and ``c`` complex128, an Ensemble's ``(t, k,
        c[rows, nsys, nmodes])`` with ``k [nsys, nmodes]`` when the members have grids of their own, of
        this rank's members only; the fields never come to the host for it."""
        self._add_observer("_spectra", name, expression, modes, every, capacity)

    def remove_spectrum(self, name):
        self._observer_set_of("_spectra", name).remove(name)

    @property
    def spectra(self):
        """name -> (t, k, c): float64 times and wavenumbers, one complex128 row of c per recorded state."""
        return self._series("_spectra")

    # ---- device extrema (extrema.py) ----------------------------------------------------
    def add_extrema(self, name, expression, kind="max", threshold=None, every=1, max_count=256, capacity=None,
                    refine=True):
        """Record the local extrema of the model expression ``expression`` (``v`` at the nodes ``g = 0 ...
        N - 1``) on the GPU (``extrema.py``): node ``g`` is a "max" iff ``v[g-1] < v[g] > v[g+1]``,
        strictly (a "min": reversed), ``v[g]`` is finite and, with a ``threshold``, ``v[g] > threshold``
        (a "min": ``<``) -- ``scipy.signal.argrelextrema(v, np.greater, mode="wrap")`` on a periodic grid,
        ``mode="clip"`` on any other (nodes ``0`` and ``N - 1`` are never extrema there).  A NaN compares
        false; a plateau of exactly equal values is not reported.  A row now, then after every
        ``every``-th step (a Simulation: where the post-processes run); ``capacity``: rows of the ring in
        device memory (default 1024, or what 32 MB hold).  The series is ``extrema[name] = (t, n, g, x,
        v)``: ``n[rows]`` (int64) the number of extrema found, which may exceed ``max_count``; the first
        ``min(n, max_count)`` in ascending node order: ``g[rows, max_count]`` (int64) the node, -1 past
        them, ``x`` and ``v`` (float64, NaN past them) the vertex of the parabola through the node and its
        neighbours (``refine=True``) or the node's own ``x`` and ``v[g]`` (``refine=False``).  An
        Ensemble's: ``n[rows, nsys]`` and ``g, x, v [rows, nsys, max_count]``, of this rank's members only;
        the fields never come to the host for it."""
        self._add_observer("_extrema", name, expression, kind, threshold, every, max_count, capacity, refine)

    def remove_extrema(self, name):
        self._observer_set_of("_extrema", name).remove(name)

    @property
    def extrema(self):
        """name -> (t, n, g, x, v): float64 times, int64 counts and nodes, float64 positions and values,
        one row per recorded state."""
        return self._series("_extrema")

    # ---- device histograms (histograms.py) ------------------------------------------------
    def add_histogram(self, name, expression, bins, range=None, every=1, nodes=slice(None), capacity=None):
        """Record the distribution of the values ``v`` of the model expression ``expression`` at the nodes
        ``nodes`` (a slice with a step >= 1) on the GPU (``histograms.py``).  ``bins``: an integer ``1 ...
        histograms.MAX_BINS`` with ``range=(lo, hi)`` -- the edges are ``np.linspace(lo, hi, bins + 1)`` --
        or a 1-D array of ``2 ... MAX_BINS + 1`` finite, strictly increasing edges (``range=None``); there
        is no automatic range.  Bin ``i`` counts ``edges[i] <= v < edges[i + 1]``, the last bin also
        ``v == edges[-1]``: ``np.histogram(v, bins, range)[0]``, exactly.  A row now, then after every
        ``every``-th step (a Simulation: where the post-processes run); ``capacity``: rows of the ring in
        device memory (default 1024).  The series is ``histograms[name] = (t, edges, counts[rows, nbins],
        outside[rows, 3])`` with int64 counts and ``outside = (below, above, nan)`` the nodes with ``v <
        edges[0]``, ``v > edges[-1]`` and ``v != v``: every row sums to the number of window nodes.  An
        Ensemble's: ``counts[rows, nsys, nbins]`` and ``outside[rows, nsys, 3]``, one ``edges`` for all
        members, of this rank's members only; the fields never come to the host for it.  Nothing is
        accumulated over time on the device: that is ``counts.sum(0)``."""
        self._add_observer("_histograms", name, expression, bins, range, every, nodes, capacity)

    def remove_histogram(self, name):
        self._observer_set_of("_histograms", name).remove(name)

    @property
    def histograms(self):
        """name -> (t, edges, counts, outside): float64 times and edges, int64 counts, one row per
        recorded state."""
        return self._series("_histograms")
