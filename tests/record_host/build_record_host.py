"""TEST-ONLY: build and drive the host harness of the device recorders (record_host.cpp).

Built by tests/observer_host/common.py from the record block (codegen.lower_records) and csrc/tf_record.h
into tests/record_host/_build/record_<hash>.so.  ``Harness.row`` returns one row of a recorder of one
system.  The triflow_amd package never loads it.
"""
import os

import numpy as np

from tests.observer_host import common
from triflow_amd import codegen, probes

HERE = os.path.dirname(os.path.abspath(__file__))
HEADERS = ("tf_args.h", "tf_math.h", "tf_layout.h", "tf_kernels.h", "tf_node.h", "tf_record.h")


def build(model, exprs, parvec_mask=0):
    """Returns (ctypes library, record spec) for these expressions of ``model``."""
    disc = [probes.discretise(model, e) for e in exprs]
    block, spec = codegen.lower_records(model, disc, parvec_mask=parvec_mask)
    return common.build(model, block, os.path.join(HERE, "record_host.cpp"), HEADERS, parvec_mask), spec


class Harness:
    """The recorders ``exprs`` of ``model`` on one system: ``row(which, pool, nodes)`` -> [ncols]."""

    def __init__(self, model, exprs, x, fields, pars, periodic, P, parvec_mask=0):
        self.lib, spec = build(model, exprs, parvec_mask)
        self.L, self.arrays = common.system_planes(model, spec, x, fields, pars, periodic, P, parvec_mask)
        self.N = self.L.N

    def row(self, which, pool, nodes):
        start, stop, step = nodes.indices(self.N)
        out = np.zeros(-(-(stop - start) // step))
        self.lib.record_host_run(common.C.byref(self.L), *[common.dptr(a) for a in self.arrays], int(which),
                                 codegen.RECORD_POOLS.index(pool), start, stop, step, common.dptr(out))
        return out
