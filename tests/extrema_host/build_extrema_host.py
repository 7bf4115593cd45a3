"""TEST-ONLY: build and drive the host harness of the device extrema (extrema_host.cpp).

Built by tests/observer_host/common.py from the extrema block (codegen.lower_extrema) and
csrc/tf_extrema.h into tests/extrema_host/_build/extrema_<hash>.so.  ``Harness.run`` computes one row of
one system as the two kernels do.  The triflow_amd package never loads it.
"""
import ctypes as C
import os

import numpy as np

from tests.observer_host import common
from triflow_amd import codegen, probes
from triflow_amd.extrema import EXTREMA_KINDS

HERE = os.path.dirname(os.path.abspath(__file__))
HEADERS = ("tf_args.h", "tf_math.h", "tf_layout.h", "tf_kernels.h", "tf_node.h", "tf_extrema.h")


def build(model, exprs, parvec_mask=0):
    """Returns (ctypes library, extrema spec) for these expressions of ``model``."""
    disc = [probes.discretise(model, e) for e in exprs]
    block, spec = codegen.lower_extrema(model, disc, parvec_mask=parvec_mask)
    lib = common.build(model, block, os.path.join(HERE, "extrema_host.cpp"), HEADERS, parvec_mask)
    lib.extrema_host_is.argtypes = [C.c_int] + [C.c_double] * 4
    return lib, spec


class Harness:
    """The extrema of ``exprs`` of ``model`` on one system of ``x.size`` nodes in ``P`` chunks."""

    def __init__(self, model, exprs, x, pars, periodic, P, parvec_mask=0):
        self.model, self.x, self.pars, self.periodic, self.P, self.mask = model, x, pars, periodic, P, parvec_mask
        self.lib, self.spec = build(model, exprs, parvec_mask)
        self.walks = 0

    def run(self, which, fields, kind="max", threshold=None, max_count=256):
        """Row of expression ``which`` for the state ``fields`` (dict of [N] arrays) -> ``(n, g [k], triples
        [k][3])`` with ``k = min(n, max_count)``; the entries past ``k`` stay the -7.0 the row was filled
        with (asserted here).  ``walks``: the threads that walked twice."""
        L, planes = common.system_planes(self.model, self.spec, self.x, fields, self.pars, self.periodic,
                                         self.P, self.mask)
        if threshold is None:
            threshold = -np.inf if kind == "max" else np.inf
        out = np.full(1 + 4 * max_count, -7.0)
        walks = C.c_int(0)
        rc = self.lib.extrema_host_run(C.byref(L), *[common.dptr(a) for a in planes], int(which),
                                       EXTREMA_KINDS.index(kind), C.c_double(threshold), int(max_count),
                                       common.dptr(out), C.byref(walks))
        assert rc == 0
        self.walks = walks.value
        n = int(out[0])
        assert n == out[0] and n >= 0
        k = min(n, max_count)
        ent = out[1:].reshape(max_count, 4)
        assert (ent[k:] == -7.0).all()
        return n, ent[:k, 0].astype(np.int64), ent[:k, 1:].copy()
