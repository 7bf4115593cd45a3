"""TEST-ONLY: build and drive the host harness of the device probes (probe_host.cpp).

The model's generated translation unit (codegen.lower_model) and the probe block
(codegen.lower_probes) are compiled with g++ together with csrc/tf_kernels.h and csrc/tf_probe.h,
``TF_DEVICE`` as ``static inline`` (as tests/emu does for the solver kernels), into
tests/probe_host/_build/probe_<hash>.so.  ``run`` lays the inputs out in the partition-interleaved
planes of a solver level (TfLayout, csrc/tf_args.h) and returns the per-node probe values and the
finished reductions.  The triflow_amd package never loads it.
"""
import ctypes as C
import os
import subprocess

import numpy as np

from triflow_amd import codegen, probes

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
CSRC = os.path.join(ROOT, "triflow_amd", "csrc")
BUILD = os.path.join(HERE, "_build")


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


def build(model, exprs, reductions, parvec_mask=0):
    """Returns (ctypes library, probe spec) for these probes of ``model``."""
    disc = [probes.discretise(model, e) for e in exprs]
    body, _ = codegen.lower_model(model, parvec_mask=parvec_mask)
    block, spec = codegen.lower_probes(model, disc, reductions, parvec_mask=parvec_mask)
    src = body + block
    deps = []
    for name in ("tf_args.h", "tf_math.h", "tf_kernels.h", "tf_probe.h"):
        with open(os.path.join(CSRC, name), "rb") as f:
            deps.append(f.read())
    with open(os.path.join(HERE, "probe_host.cpp"), "rb") as f:
        deps.append(f.read())
    tag = codegen.source_hash(src, *deps)
    os.makedirs(BUILD, exist_ok=True)
    so = os.path.join(BUILD, "probe_%s.so" % tag)
    if not os.path.exists(so):
        hdr = os.path.join(BUILD, "probe_%s.h" % tag)
        with open(hdr + ".%d.tmp" % os.getpid(), "w") as f:
            f.write(src)
        os.replace(hdr + ".%d.tmp" % os.getpid(), hdr)
        tmp = so + ".%d.tmp" % os.getpid()
        cmd = ["g++", "-std=c++17", "-O1", "-g0", "-shared", "-fPIC", "-ffp-contract=off", "-fno-fast-math",
               "-I", CSRC, '-DTF_PROBE_HOST_HEADER="%s"' % hdr, os.path.join(HERE, "probe_host.cpp"), "-o", tmp]
        res = subprocess.run(cmd, capture_output=True, text=True)
        if res.returncode != 0:
            raise RuntimeError("probe harness build failed:\n" + res.stderr[-4000:])
        os.replace(tmp, so)
    return C.CDLL(so), spec


def run(model, exprs, reductions, x, fields, pars, periodic, P, parvec_mask=0):
    """Per-node values [nprobe][N] and reductions [nprobe] of one system (``fields``: dict of
    [N] arrays, dependent variables and help functions; ``pars``: dict of scalars / [N] arrays)."""
    lib, spec = build(model, exprs, reductions, parvec_mask)
    x = np.asarray(x, dtype=float)
    N = x.size
    L = layout(1, N, P, periodic)
    names = list(model._dep_vars)
    helps = list(model._help_funcs)
    parnames = list(model._pars)
    fplanes = np.concatenate([to_plane(L, fields[k]) for k in names])
    hplanes = np.concatenate([to_plane(L, fields[k]) for k in helps]) if helps else np.zeros(1)
    pv = [np.asarray(pars[k], dtype=float) for k in parnames]
    parvec = np.concatenate([to_plane(L, v) for v in pv]) if parvec_mask else np.zeros(1)
    dx = (x[-1] - x[0]) / (N - 1)
    hc_model = codegen.eval_host_constants(
        codegen.lower_model(model, parvec_mask=parvec_mask)[1], dx, pv)
    parsca = np.array([float(np.ravel(v)[0]) for v in pv] + hc_model + [0.0])
    hc = np.array(codegen.eval_host_constants(spec, dx, pv) + [0.0])
    xplane = to_plane(L, x)
    nprobe = spec["nprobe"]
    out = np.zeros(nprobe)
    nodes = np.zeros((nprobe, N))
    d = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    dxa = np.array([dx])
    lib.probe_host_run(C.byref(L), d(fplanes), d(hplanes), d(parvec), d(parsca), d(dxa), d(xplane),
                       d(hc), d(out), d(nodes))
    return nodes, out
