"""TEST-ONLY: build and drive the host harness of the device histograms (hist_host.cpp).

Built by tests/observer_host/common.py from the histogram block (codegen.lower_histograms) and
csrc/tf_histogram.h into tests/hist_host/_build/hist_<hash>.so.  ``Harness.run`` computes one row of one
system as the two kernels do, ``classify`` is the kernels' classification alone.
The triflow_amd package never loads it.
"""
import ctypes as C
import os

import numpy as np

from tests.observer_host import common
from triflow_amd import codegen, probes

HERE = os.path.dirname(os.path.abspath(__file__))
HEADERS = ("tf_args.h", "tf_math.h", "tf_layout.h", "tf_kernels.h", "tf_node.h", "tf_histogram.h")


def build(model, exprs, parvec_mask=0):
    """Returns (ctypes library, histogram spec) for these expressions of ``model``."""
    disc = [probes.discretise(model, e) for e in exprs]
    block, spec = codegen.lower_histograms(model, disc, parvec_mask=parvec_mask)
    return common.build(model, block, os.path.join(HERE, "hist_host.cpp"), HEADERS, parvec_mask), spec


def classify(lib, v, edges):
    """The counter of the value ``v``: 0 ... nbins - 1, then below, above, NaN."""
    e = np.ascontiguousarray(edges, dtype=float)
    return lib.hist_host_classify(C.c_double(float(v)), common.dptr(e), int(e.size - 1))


class Harness:
    """The histograms ``exprs`` of ``model`` on one system of ``x.size`` nodes in ``P`` chunks."""

    def __init__(self, model, exprs, x, pars, periodic, P, parvec_mask=0):
        self.model, self.x, self.pars, self.periodic, self.P, self.mask = model, x, pars, periodic, P, parvec_mask
        self.lib, self.spec = build(model, exprs, parvec_mask)
        self.sets = 0                # workgroups of tfk_hist_partial in the last run

    def run(self, which, edges, fields, nodes=slice(None), window=None):
        """Row of expression ``which`` for the state ``fields`` (dict of [N] arrays): ``(counts [nbins],
        outside [3])`` int64.  ``window``: (start, stop, step) as is, instead of ``nodes.indices(N)``."""
        L, planes = common.system_planes(self.model, self.spec, self.x, fields, self.pars, self.periodic,
                                         self.P, self.mask)
        e = np.ascontiguousarray(edges, dtype=float)
        nbins = e.size - 1
        start, stop, step = window or nodes.indices(L.N)
        out = np.zeros(nbins + 3)
        sets = C.c_int(0)
        rc = self.lib.hist_host_run(C.byref(L), *[common.dptr(a) for a in planes], int(which), int(nbins),
                                    common.dptr(e), int(start), int(stop), int(step), common.dptr(out),
                                    C.byref(sets))
        assert rc == 0
        self.sets = sets.value
        assert (out == np.floor(out)).all()
        return out[:nbins].astype(np.int64), out[nbins:].astype(np.int64)
