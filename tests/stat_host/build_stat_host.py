"""TEST-ONLY: build and drive the host harness of the device statistics (stat_host.cpp).

Built by tests/observer_host/common.py from the statistic block (codegen.lower_statistics) and
csrc/tf_stat.h into tests/stat_host/_build/stat_<hash>.so.  ``Harness.update`` folds one state (``Harness.state``) of one
system into the accumulator planes of a statistic, ``Harness.natural`` brings planes back to node order.
The triflow_amd package never loads it.
"""
import os

import numpy as np

from tests.observer_host import common
from triflow_amd import codegen, probes
from triflow_amd.statistics import STATISTIC_KINDS

HERE = os.path.dirname(os.path.abspath(__file__))
HEADERS = ("tf_args.h", "tf_math.h", "tf_layout.h", "tf_kernels.h", "tf_node.h", "tf_stat.h")


def build(model, exprs, parvec_mask=0):
    """Returns (ctypes library, statistic spec) for these expressions of ``model``."""
    disc = [probes.discretise(model, e) for e in exprs]
    block, spec = codegen.lower_statistics(model, disc, parvec_mask=parvec_mask)
    return common.build(model, block, os.path.join(HERE, "stat_host.cpp"), HEADERS, parvec_mask), spec


class Harness:
    """The statistics ``exprs`` of ``model`` on one system of ``x.size`` nodes in ``P`` chunks."""

    def __init__(self, model, exprs, x, pars, periodic, P, parvec_mask=0):
        self.model, self.x, self.pars, self.periodic, self.P, self.mask = model, x, pars, periodic, P, parvec_mask
        self.lib, self.spec = build(model, exprs, parvec_mask)
        self.L = common.layout(1, np.asarray(x).size, P, periodic)

    def planes(self, kind):
        """Fresh accumulators of a statistic of ``kind``, filled with a value no sample has (sample 1
        must overwrite them)."""
        return np.full(self.lib.stat_host_planes(STATISTIC_KINDS.index(kind)) * self.L.plane, -7.25)

    def state(self, fields):
        """The inputs of an update for the state ``fields`` (dict of [N] arrays), laid out once."""
        return common.system_planes(self.model, self.spec, self.x, fields, self.pars, self.periodic,
                                    self.P, self.mask)[1]

    def update(self, which, kind, k, t, state, acc):
        """``state`` (of ``self.state``) as sample ``k`` at ``t`` into ``acc``."""
        self.lib.stat_host_update(common.C.byref(self.L), *[common.dptr(a) for a in state], int(which),
                                  STATISTIC_KINDS.index(kind), common.C.c_double(k), common.C.c_double(t),
                                  common.dptr(acc))

    def natural(self, acc):
        """[planes * plane] partition-interleaved -> [planes][N] in node order."""
        L = self.L
        out = np.zeros((acc.size // L.plane, L.N))
        for c in range(out.shape[0]):
            for p in range(L.P):
                start = p * L.mbase + min(p, L.rem)
                ln = L.mbase + (p < L.rem)
                out[c, start:start + ln] = acc[c * L.plane + np.arange(ln) * L.Ptot + p]
        return out
