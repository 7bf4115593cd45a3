"""TEST-ONLY: build and drive the host harness of the device spectra (spectrum_host.cpp).

Built by tests/observer_host/common.py from the spectrum block (codegen.lower_spectra) and
csrc/tf_spectrum.h into tests/spectrum_host/_build/spectrum_<hash>.so.  ``Harness.run`` computes one row
of one system as the two kernels do, ``twiddle`` is the kernels' twiddle function alone.
The triflow_amd package never loads it.
"""
import ctypes as C
import os

import numpy as np

from tests.observer_host import common
from triflow_amd import codegen, probes

HERE = os.path.dirname(os.path.abspath(__file__))
HEADERS = ("tf_args.h", "tf_math.h", "tf_layout.h", "tf_kernels.h", "tf_node.h", "tf_spectrum.h")


def build(model, exprs, parvec_mask=0):
    """Returns (ctypes library, spectrum spec) for these expressions of ``model``."""
    disc = [probes.discretise(model, e) for e in exprs]
    block, spec = codegen.lower_spectra(model, disc, parvec_mask=parvec_mask)
    return common.build(model, block, os.path.join(HERE, "spectrum_host.cpp"), HEADERS, parvec_mask), spec


def twiddle(lib, r, N):
    """exp(-2 pi i r / N) of the kernels' twiddle function: (re, im)."""
    out = np.zeros(2)
    lib.spectrum_host_twiddle(C.c_int64(int(r)), C.c_int64(int(N)), common.dptr(out))
    return out[0], out[1]


class Harness:
    """The spectra ``exprs`` of ``model`` on one system of ``x.size`` nodes in ``P`` chunks."""

    def __init__(self, model, exprs, x, pars, periodic, P, parvec_mask=0):
        self.model, self.x, self.pars, self.periodic, self.P, self.mask = model, x, pars, periodic, P, parvec_mask
        self.lib, self.spec = build(model, exprs, parvec_mask)

    def run(self, which, modes, fields):
        """Row of expression ``which`` at ``modes`` for the state ``fields`` (dict of [N] arrays):
        complex128 [nmodes]."""
        L, planes = common.system_planes(self.model, self.spec, self.x, fields, self.pars, self.periodic,
                                         self.P, self.mask)
        m = np.ascontiguousarray(modes, dtype=np.int32)
        out = np.zeros(2 * m.size)
        rc = self.lib.spectrum_host_run(C.byref(L), *[common.dptr(a) for a in planes], int(which), int(m.size),
                                        m.ctypes.data_as(C.POINTER(C.c_int32)), common.dptr(out))
        assert rc == 0
        return out.view(np.complex128)
