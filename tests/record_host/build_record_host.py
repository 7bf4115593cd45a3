"""TEST-ONLY: build and drive the host harness of the device recorders (record_host.cpp).

The model's generated translation unit (codegen.lower_model) and the record block
(codegen.lower_records) are compiled with g++ together with csrc/tf_kernels.h, csrc/tf_probe.h and
csrc/tf_record.h, ``TF_DEVICE`` as ``static inline`` (the pattern of tests/probe_host), into
tests/record_host/_build/record_<hash>.so.  ``run`` lays the inputs out in the partition-interleaved
planes of a solver level and returns one row of a recorder.  The triflow_amd package never loads it.
"""
import ctypes as C
import os
import subprocess

import numpy as np

from tests.probe_host.build_probe_host import layout, to_plane
from triflow_amd import codegen, probes

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
CSRC = os.path.join(ROOT, "triflow_amd", "csrc")
BUILD = os.path.join(HERE, "_build")


def build(model, exprs, parvec_mask=0):
    """Returns (ctypes library, record spec) for these expressions of ``model``."""
    disc = [probes.discretise(model, e) for e in exprs]
    body, _ = codegen.lower_model(model, parvec_mask=parvec_mask)
    block, spec = codegen.lower_records(model, disc, parvec_mask=parvec_mask)
    src = body + block
    deps = []
    for name in ("tf_args.h", "tf_math.h", "tf_kernels.h", "tf_probe.h", "tf_record.h"):
        with open(os.path.join(CSRC, name), "rb") as f:
            deps.append(f.read())
    with open(os.path.join(HERE, "record_host.cpp"), "rb") as f:
        deps.append(f.read())
    tag = codegen.source_hash(src, *deps)
    os.makedirs(BUILD, exist_ok=True)
    so = os.path.join(BUILD, "record_%s.so" % tag)
    if not os.path.exists(so):
        hdr = os.path.join(BUILD, "record_%s.h" % tag)
        with open(hdr + ".%d.tmp" % os.getpid(), "w") as f:
            f.write(src)
        os.replace(hdr + ".%d.tmp" % os.getpid(), hdr)
        tmp = so + ".%d.tmp" % os.getpid()
        cmd = ["g++", "-std=c++17", "-O1", "-g0", "-shared", "-fPIC", "-ffp-contract=off", "-fno-fast-math",
               "-I", CSRC, '-DTF_RECORD_HOST_HEADER="%s"' % hdr, os.path.join(HERE, "record_host.cpp"), "-o", tmp]
        res = subprocess.run(cmd, capture_output=True, text=True)
        if res.returncode != 0:
            raise RuntimeError("record harness build failed:\n" + res.stderr[-4000:])
        os.replace(tmp, so)
    return C.CDLL(so), spec


class Harness:
    """The recorders ``exprs`` of ``model`` on one system: ``row(which, pool, nodes)`` -> [ncols]."""

    def __init__(self, model, exprs, x, fields, pars, periodic, P, parvec_mask=0):
        self.lib, spec = build(model, exprs, parvec_mask)
        x = np.asarray(x, dtype=float)
        self.N = x.size
        self.L = layout(1, self.N, P, periodic)
        helps = list(model._help_funcs)
        pv = [np.asarray(pars[k], dtype=float) for k in model._pars]
        dx = (x[-1] - x[0]) / (self.N - 1)
        hc_model = codegen.eval_host_constants(codegen.lower_model(model, parvec_mask=parvec_mask)[1], dx, pv)
        self.arrays = [
            np.concatenate([to_plane(self.L, fields[k]) for k in model._dep_vars]),
            np.concatenate([to_plane(self.L, fields[k]) for k in helps]) if helps else np.zeros(1),
            np.concatenate([to_plane(self.L, v) for v in pv]) if parvec_mask else np.zeros(1),
            np.array([float(np.ravel(v)[0]) for v in pv] + hc_model + [0.0]),
            np.array([dx]),
            to_plane(self.L, x),
            np.array(codegen.eval_host_constants(spec, dx, pv) + [0.0])]

    def row(self, which, pool, nodes):
        start, stop, step = nodes.indices(self.N)
        out = np.zeros(-(-(stop - start) // step))
        d = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
        self.lib.record_host_run(C.byref(self.L), *[d(a) for a in self.arrays], int(which),
                                 codegen.RECORD_POOLS.index(pool), start, stop, step, d(out))
        return out
