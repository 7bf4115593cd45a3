"""Device observers: what the probes (``probes.py``), the recorders (``recorders.py``), the statistics
(``statistics.py``), the spectra (``spectra.py``), the extrema (``extrema.py``) and the histograms
(``histograms.py``) share.

An observer evaluates expressions in the model's own string language at the nodes of a resident state
slot and writes one row per record into a ring in device memory.  Both kinds go through the same node
core (``csrc/tf_node.h``): the expressions are discretised with the model's stencils (``discretise``),
lowered to a block of C that follows the model's translation unit, and compiled into one more code
object of the model (``compilers.build_observer_code_object``); a handle per solver binds it
(``_capi.DeviceProbe`` / ``DeviceRecord``) and is fed ``x`` and the host constants of the expressions.
:class:`ObserverSet` owns that part.  A kind of observer supplies the lowering of its expressions, its
handle, and what a row is.
"""

import numpy as np
import sympy as sp
from sympy.core.function import AppliedUndef

from . import codegen
from .codegen import UnsupportedExpression

__all__ = ["ObserverSet", "Observed", "discretise"]


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
    "record" / "stat" / "spectrum" / "extrema" / "histogram": ``compilers.build_observer_code_object``), ``_lower(mask) -> (block, spec)``,
    ``_make_handle(solver, code, spec)`` and ``_flush()`` (every row still on the device to the series)."""

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


class Observed:
    """``add_probe`` / ``add_recorder`` / ``add_statistic`` / ``add_spectrum`` / ``add_extrema`` /
    ``add_histogram`` ... of a front end (``Simulation``, ``Ensemble``): reductions over space, decimated
    space-time pictures, reductions over time, Fourier amplitudes, the crests and troughs and the
    distribution of values over time.  The front end
    has ``model``, says how a set records its current state (``_record_on(series_set)``: also called after
    every step for ``_probes``, ``_recorders``, ``_statistics``, ``_spectra``, ``_extrema`` and ``_histograms`` that are not None), how many nodes a system has
    (``_n_nodes``) and whether its series keep the axis of the systems (``_per_system``)."""

    _probes = _recorders = _statistics = _spectra = _extrema = _histograms = None
    _per_system = True

    def _add_observer(self, series_set, name, *args):
        series_set.add(name, *args)
        try:
            self._record_on(series_set)
        except Exception:
            # (no code object / no handle for the new set: the new one is not kept, the others go on)
            series_set.remove(name)
            raise

    # ---- device probes (probes.py) ----------------------------------------------------
    def add_probe(self, name, expression, reduce="sum"):
        """Record ``reduce`` of the model expression ``expression`` over the nodes (of every member of
        an ensemble) after every step, on the GPU (``probes.py``): the t0 row now, then one row after
        every step (a Simulation: where the post-processes run).  The series is ``probes[name] =
        (t, values)``, an Ensemble's ``(t, values[rows, nsys])`` of this rank's members only; the
        fields are never brought to the host for it."""
        if self._probes is None:
            from .probes import ProbeSet
            self._probes = ProbeSet(self.model)
        self._add_observer(self._probes, name, expression, reduce)

    def remove_probe(self, name):
        if self._probes is None:
            raise KeyError(name)
        self._probes.remove(name)

    @property
    def probes(self):
        """name -> (t, values): float64 arrays, one entry per recorded state."""
        return self._probes.series(per_system=self._per_system) if self._probes is not None else {}

    # ---- device recorders (recorders.py) ----------------------------------------------
    def add_recorder(self, name, expression, every=1, nodes=slice(None), pool="sample", capacity=None):
        """Record the model expression ``expression`` on the GPU at the columns ``nodes`` (a slice; a
        column is the ``pool`` -- "sample", "max", "min", "mean" -- of a bin of ``nodes.step`` nodes):
        a row now, then after every ``every``-th step (a Simulation: where the post-processes run).
        The series is ``recorders[name] = (t, x, values[rows, ncols])``, an Ensemble's ``(t, x,
        values[rows, nsys, ncols])`` with ``x [nsys, ncols]`` when the members have grids of their own,
        of this rank's members only; the fields never come to the host for it."""
        if self._recorders is None:
            from .recorders import RecorderSet
            self._recorders = RecorderSet(self.model, self._n_nodes)
        self._add_observer(self._recorders, name, expression, every, nodes, pool, capacity)

    def remove_recorder(self, name):
        if self._recorders is None:
            raise KeyError(name)
        self._recorders.remove(name)

    @property
    def recorders(self):
        """name -> (t, x, values): float64 arrays, one row of values per recorded state."""
        return self._recorders.series(per_system=self._per_system) if self._recorders is not None else {}

    # ---- device statistics (statistics.py) --------------------------------------------
    def add_statistic(self, name, expression, stat="mean", every=1, nodes=slice(None)):
        """Accumulate the statistic ``stat`` -- "mean", "var", "max", "min", "argmax", "argmin" (the
        ``t`` of the first extremal sample) -- over time of the model expression ``expression`` at every
        node, on the GPU (``statistics.py``): the current state is sample 1, then the state after every
        ``every``-th step is a sample (a Simulation: where the post-processes run), all of one weight.
        ``statistics[name] = (n, x, values[ncols])`` at the nodes ``nodes`` (a slice), an Ensemble's
        ``(n, x, values[nsys, ncols])`` of this rank's members only; the fields never come to the host
        for it."""
        if self._statistics is None:
            from .statistics import StatisticSet
            self._statistics = StatisticSet(self.model, self._n_nodes)
        self._add_observer(self._statistics, name, expression, stat, every, nodes)

    def remove_statistic(self, name):
        if self._statistics is None:
            raise KeyError(name)
        self._statistics.remove(name)

    def reset_statistic(self, name):
        """Drop the samples taken so far (a transient): the next due state is sample 1 again."""
        if self._statistics is None:
            raise KeyError(name)
        self._statistics.reset(name)

    @property
    def statistics(self):
        """name -> (n, x, values): the samples folded so far, float64 arrays over the nodes."""
        return self._statistics.series(per_system=self._per_system) if self._statistics is not None else {}

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
        if self._spectra is None:
            from .spectra import SpectrumSet
            self._spectra = SpectrumSet(self.model, self._n_nodes)
        self._add_observer(self._spectra, name, expression, modes, every, capacity)

    def remove_spectrum(self, name):
        if self._spectra is None:
            raise KeyError(name)
        self._spectra.remove(name)

    @property
    def spectra(self):
        """name -> (t, k, c): float64 times and wavenumbers, one complex128 row of c per recorded state."""
        return self._spectra.series(per_system=self._per_system) if self._spectra is not None else {}

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
        if self._extrema is None:
            from .extrema import ExtremaSet
            self._extrema = ExtremaSet(self.model, self._n_nodes)
        self._add_observer(self._extrema, name, expression, kind, threshold, every, max_count, capacity, refine)

    def remove_extrema(self, name):
        if self._extrema is None:
            raise KeyError(name)
        self._extrema.remove(name)

    @property
    def extrema(self):
        """name -> (t, n, g, x, v): float64 times, int64 counts and nodes, float64 positions and values,
        one row per recorded state."""
        return self._extrema.series(per_system=self._per_system) if self._extrema is not None else {}

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
        if self._histograms is None:
            from .histograms import HistogramSet
            self._histograms = HistogramSet(self.model, self._n_nodes)
        self._add_observer(self._histograms, name, expression, bins, range, every, nodes, capacity)

    def remove_histogram(self, name):
        if self._histograms is None:
            raise KeyError(name)
        self._histograms.remove(name)

    @property
    def histograms(self):
        """name -> (t, edges, counts, outside): float64 times and edges, int64 counts, one row per
        recorded state."""
        return self._histograms.series(per_system=self._per_system) if self._histograms is not None else {}
