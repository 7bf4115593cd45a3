"""Device spectra: amplitudes of chosen Fourier modes of model expressions, computed where the state lives.

A spectrum is a named expression in the model's own string language (what a probe accepts:
``observers.discretise``), a list of integer modes ``m_i`` in ``0 ... N // 2`` and a stride in steps
``every``.  A row is ``c[i] = sum_g v_g * exp(-2j * pi * m_i * g / N)`` over the nodes ``g = 0 ... N - 1``
of a system, ``v`` the expression at the nodes: ``np.fft.fft(v)[m_i]``, unnormalised, no window, nothing
subtracted (write ``h - 1``).  A grid that is not periodic gets the same sum over its node sequence.  The
wavenumber of mode ``m`` is ``k = 2 * pi * m / (N * dx)``.  The expressions are lowered by
``codegen.lower_spectra`` and compiled into one more code object of the model (``observers.py``: what the
spectra share with the probes, the recorders and the statistics); the spectrum kernels
(``csrc/tf_spectrum.h``) read a resident state slot once per record and write one row into the spectrum's
ring in device memory, which comes to the host when it is full and when the series is read
(``tf_spectrum_*``).  The modes are data of the handle: spectra of the same expressions share a code
object whatever their modes.

:class:`SpectrumSet` is what ``Simulation.add_spectrum`` and ``Ensemble.add_spectrum`` build on.
"""

import numpy as np

from . import codegen
from .observers import RowItem, RowObserverSet, _is_int, checked_capacity, checked_every, discretise
from .observers import _Bound  # noqa: F401  (the tests build one)

__all__ = ["SpectrumSet", "MAX_MODES", "DEFAULT_CAPACITY", "MAX_SPECTRA"]

#: modes of one spectrum (TF_SPEC_MAX_MODES of csrc/tf_args.h).  A workgroup of tfk_spectrum_partial keeps
#: 192 bytes of tables per mode in LDS (8 step twiddles and the sums of its 4 wavefronts, complex doubles).
#: A CU holds 8 such workgroups and 160 KiB of LDS: 20 KiB each, 106 modes; 64 is the power of two below,
#: so the tables never decide how many workgroups are resident.  More modes: a second spectrum.
MAX_MODES = 64
#: rows of the device ring of a spectrum: a run waits for the GPU once per this many records
DEFAULT_CAPACITY = 1024
#: spectra of one set (tf_spectrum_create)
MAX_SPECTRA = 64


class _Spectrum(RowItem):
    def __init__(self, name, expression, disc, modes, every, capacity):
        super().__init__(name, expression, disc, every)    # (a row: [nsys][nmodes], complex)
        self.modes, self.capacity = modes, capacity
        self.k = None                # [nmodes] or [nsys][nmodes]


class SpectrumSet(RowObserverSet):
    """The spectra of one Simulation or Ensemble (``N`` nodes per system) and their series.

    Rows are recorded on the device (``record``) and fetched when the series are read (``series``):
    one ``tf_spectrum`` handle per solver the set has run on, one code object per parameter layout /
    sweep segment of those solvers."""

    kind = "spectrum"
    _laid_out = "the spectrum modes were laid out for"

    # ---- the set ---------------------------------------------------------------------
    def _modes(self, name, modes):
        try:
            given = list(modes)
        except TypeError:
            raise ValueError("spectrum %r: modes=%r, a sequence of integers is expected" % (name, modes))
        if not given:
            raise ValueError("spectrum %r: modes is empty" % (name,))
        for m in given:
            if not _is_int(m):
                raise ValueError("spectrum %r: mode %r is not an integer" % (name, m))
        given = [int(m) for m in given]
        if len(given) > MAX_MODES:
            raise ValueError("spectrum %r: %d modes, at most %d per spectrum (add a second spectrum)"
                             % (name, len(given), MAX_MODES))
        for m in given:
            if m < 0 or m > self.N // 2:
                raise ValueError("spectrum %r: mode %d is outside 0 ... N // 2 = %d (a real signal's modes "
                                 "above are the conjugates of those below)" % (name, m, self.N // 2))
        if len(set(given)) != len(given):
            raise ValueError("spectrum %r: modes=%r names a mode twice" % (name, given))
        return given

    def add(self, name, expression, modes, every=1, capacity=None):
        """Validate, lower and append one spectrum (nothing is computed yet)."""
        if name in self.names:
            raise ValueError("a spectrum named %r exists already" % (name,))
        every = checked_every("spectrum", name, every)
        modes = self._modes(name, modes)
        capacity = checked_capacity("spectrum", name, capacity)
        if len(self._items) >= MAX_SPECTRA:
            raise ValueError("at most %d spectra per simulation (spectrum %r)" % (MAX_SPECTRA, name))
        disc = discretise(self.model, expression)
        codegen.lower_spectra(self.model, [disc])          # (what the C emitter refuses, refused now)
        self._flush()
        self._items.append(_Spectrum(name, expression, disc, modes, every,
                                     DEFAULT_CAPACITY if capacity is None else capacity))
        self._reset()

    # ---- device side -----------------------------------------------------------------
    def _lower(self, mask):
        return codegen.lower_spectra(self.model, self.expressions(), parvec_mask=mask)

    def _make_handle(self, solver, code, spec):
        from ._capi import DeviceSpectrum
        exprs = self.expressions()
        geometry = [(exprs.index(r.disc), len(r.modes), r.capacity) for r in self._items]
        return DeviceSpectrum(solver, code, geometry, [r.modes for r in self._items], len(spec["host_consts"]))

    def _first_row(self, r, x, solver):
        dx = (x[..., -1] - x[..., 0]) / (self.N - 1)
        r.k = 2.0 * np.pi * np.asarray(r.modes, dtype=float) / (self.N * np.asarray(dx)[..., None])

    def _no_rows(self, r):
        return np.zeros((0, r.nsys, len(r.modes)), dtype=np.complex128)

    def series(self, per_system=True):
        """name -> (t [rows], k [nmodes] or [nsys, nmodes], c [rows, nsys, nmodes] complex128)
        (``per_system=False``: k [nmodes], c [rows, nmodes])."""
        self._flush()
        out = {}
        for r in self._items:
            c = self._rows(r)
            k = np.zeros(len(r.modes)) if r.k is None else r.k
            if k.ndim == 2 and (not per_system or (k == k[0]).all()):
                k = k[0]
            out[r.name] = (np.array(r.t, dtype=float), k, c if per_system else c[:, 0])
        return out
