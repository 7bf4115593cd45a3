"""TEST-ONLY: what the host harnesses of the device observers share (tests/probe_host, tests/record_host).

The model's generated translation unit (codegen.lower_model) and an observer's block (codegen.lower_probes,
codegen.lower_records) are compiled with g++ together with csrc/tf_kernels.h, the node core csrc/tf_node.h
and the observer's own header, ``TF_DEVICE`` as ``static inline`` (observer_host.h; as tests/emu does for
the solver kernels), into ``_build/<name>_<hash>.so`` next to the harness source.  ``system_planes`` lays
the inputs of one system out in the partition-interleaved planes of a solver level (TfLayout,
csrc/tf_args.h).  The triflow_amd package never loads any of it.
"""
import ctypes as C
import os
import subprocess

import numpy as np

from triflow_amd import codegen

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
CSRC = os.path.join(ROOT, "triflow_amd", "csrc")


class Layout(C.Structure):
    _fields_ = [("nsys", C.c_int), ("N", C.c_int), ("P", C.c_int), ("mbase", C.c_int), ("rem", C.c_int),
                ("M", C.c_int), ("Ptot", C.c_int), ("periodic", C.c_int), ("plane", C.c_int64)]


def layout(nsys, N, P, periodic):
    mbase, rem = N // P, N % P
    M = mbase + (rem > 0)
    return Layout(nsys, N, P, mbase, rem, M, nsys * P, int(periodic), M * nsys * P)


def to_plane(L, arr):
    """[nsys][N] natural order -> one partition-interleaved plane."""
    arr = np.broadcast_to(np.asarray(arr, dtype=float), (L.nsys, L.N))
    plane = np.zeros(L.plane)
    for p in range(L.P):
        start = p * L.mbase + min(p, L.rem)
        ln = L.mbase + (p < L.rem)
        for e in range(L.nsys):
            plane[np.arange(ln) * L.Ptot + e * L.P + p] = arr[e, start:start + ln]
    return plane


def build(model, block, cpp, headers, parvec_mask=0):
    """The harness ``cpp`` (a path) for the observer block ``block`` of ``model`` -> ctypes library.
    ``headers``: the files of csrc the harness reads (they name the build, with the sources)."""
    body, _ = codegen.lower_model(model, parvec_mask=parvec_mask)
    src = body + block
    deps = []
    for path in [os.path.join(CSRC, h) for h in headers] + [os.path.join(HERE, "observer_host.h"), cpp]:
        with open(path, "rb") as f:
            deps.append(f.read())
    tag = codegen.source_hash(src, *deps)
    out = os.path.join(os.path.dirname(cpp), "_build")
    os.makedirs(out, exist_ok=True)
    name = os.path.basename(cpp)[:-len("_host.cpp")]
    so = os.path.join(out, "%s_%s.so" % (name, tag))
    if not os.path.exists(so):
        hdr = os.path.join(out, "%s_%s.h" % (name, tag))
        with open(hdr + ".%d.tmp" % os.getpid(), "w") as f:
            f.write(src)
        os.replace(hdr + ".%d.tmp" % os.getpid(), hdr)
        tmp = so + ".%d.tmp" % os.getpid()
        cmd = ["g++", "-std=c++17", "-O1", "-g0", "-shared", "-fPIC", "-ffp-contract=off", "-fno-fast-math",
               "-I", CSRC, "-I", HERE, '-DTF_OBSERVER_HOST_HEADER="%s"' % hdr, cpp, "-o", tmp]
        res = subprocess.run(cmd, capture_output=True, text=True)
        if res.returncode != 0:
            raise RuntimeError("%s harness build failed:\n%s" % (name, res.stderr[-4000:]))
        os.replace(tmp, so)
    return C.CDLL(so)


def system_planes(model, spec, x, fields, pars, periodic, P, parvec_mask=0):
    """One system (``fields``: dict of [N] arrays, dependent variables and help functions; ``pars``: dict
    of scalars / [N] arrays) -> (layout, the seven input arrays of a harness entry point in the order of
    TfNodeArgs: fields, helpers, parvec, parsca, dx, xcoord, hc).  ``spec``: the observer's."""
    x = np.asarray(x, dtype=float)
    L = layout(1, x.size, P, periodic)
    helps = list(model._help_funcs)
    pv = [np.asarray(pars[k], dtype=float) for k in model._pars]
    dx = (x[-1] - x[0]) / (x.size - 1)
    hc_model = codegen.eval_host_constants(codegen.lower_model(model, parvec_mask=parvec_mask)[1], dx, pv)
    return L, [
        np.concatenate([to_plane(L, fields[k]) for k in model._dep_vars]),
        np.concatenate([to_plane(L, fields[k]) for k in helps]) if helps else np.zeros(1),
        np.concatenate([to_plane(L, v) for v in pv]) if parvec_mask else np.zeros(1),
        np.array([float(np.ravel(v)[0]) for v in pv] + hc_model + [0.0]),
        np.array([dx]),
        to_plane(L, x),
        np.array(codegen.eval_host_constants(spec, dx, pv) + [0.0])]


def dptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))
