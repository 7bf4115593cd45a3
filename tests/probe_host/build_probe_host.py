"""TEST-ONLY: build and drive the host harness of the device probes (probe_host.cpp).

Built by tests/observer_host/common.py from the probe block (codegen.lower_probes) and csrc/tf_probe.h
into tests/probe_host/_build/probe_<hash>.so.  ``run`` returns the per-node probe values and the
finished reductions of one system.  The triflow_amd package never loads it.
"""
import os

import numpy as np

from tests.observer_host import common
from triflow_amd import codegen, probes

HERE = os.path.dirname(os.path.abspath(__file__))
HEADERS = ("tf_args.h", "tf_math.h", "tf_layout.h", "tf_kernels.h", "tf_node.h", "tf_probe.h")


def build(model, exprs, reductions, parvec_mask=0):
    """Returns (ctypes library, probe spec) for these probes of ``model``."""
    disc = [probes.discretise(model, e) for e in exprs]
    block, spec = codegen.lower_probes(model, disc, reductions, parvec_mask=parvec_mask)
    return common.build(model, block, os.path.join(HERE, "probe_host.cpp"), HEADERS, parvec_mask), spec


def run(model, exprs, reductions, x, fields, pars, periodic, P, parvec_mask=0):
    """Per-node values [nprobe][N] and reductions [nprobe] of one system (``fields``: dict of
    [N] arrays, dependent variables and help functions; ``pars``: dict of scalars / [N] arrays)."""
    lib, spec = build(model, exprs, reductions, parvec_mask)
    L, arrays = common.system_planes(model, spec, x, fields, pars, periodic, P, parvec_mask)
    out = np.zeros(spec["nprobe"])
    nodes = np.zeros((spec["nprobe"], L.N))
    lib.probe_host_run(common.C.byref(L), *[common.dptr(a) for a in arrays], common.dptr(out), common.dptr(nodes))
    return nodes, out
