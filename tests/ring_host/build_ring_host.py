"""TEST-ONLY: build and drive the host harness of the observers' ring of rows (ring_host.cpp).

g++ compiles ring_host.cpp, which includes csrc/tf_solver.h, with tests/emu/tf_backend_emu.cpp (the back
end whose device memory is the host's) and the generated header of one small model, which the emulation
needs to compile, into tests/ring_host/_build/ring_<hash>.so.  The triflow_amd package never loads it.
"""
import ctypes as C
import os
import subprocess

import numpy as np

from triflow_amd import Model, codegen

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
CSRC = os.path.join(ROOT, "triflow_amd", "csrc")
EMU = os.path.join(ROOT, "tests", "emu", "tf_backend_emu.cpp")
BUILD = os.path.join(HERE, "_build")


def build():
    src, _ = codegen.lower_model(Model("k * dxxU", "U", "k", hold_compilation=True))
    deps = []
    for path in (os.path.join(HERE, "ring_host.cpp"), EMU, os.path.join(CSRC, "tf_solver.h"),
                 os.path.join(CSRC, "tf_backend.h"), os.path.join(CSRC, "tf_args.h")):
        with open(path, "rb") as f:
            deps.append(f.read())
    tag = codegen.source_hash(src, *deps)
    so = os.path.join(BUILD, "ring_%s.so" % tag)
    if not os.path.exists(so):
        os.makedirs(BUILD, exist_ok=True)
        hdr = os.path.join(BUILD, "model_%s.h" % tag)
        with open(hdr + ".%d.tmp" % os.getpid(), "w") as f:
            f.write(src)
        os.replace(hdr + ".%d.tmp" % os.getpid(), hdr)
        tmp = so + ".%d.tmp" % os.getpid()
        cmd = ["g++", "-std=c++17", "-O1", "-g0", "-shared", "-fPIC", "-I", CSRC, "-I", os.path.join(ROOT, "include"),
               '-DTF_EMU_MODEL_HEADER="%s"' % hdr, os.path.join(HERE, "ring_host.cpp"), EMU, "-o", tmp]
        res = subprocess.run(cmd, capture_output=True, text=True)
        if res.returncode != 0:
            raise RuntimeError("ring harness build failed:\n" + res.stderr[-4000:])
        os.replace(tmp, so)
    lib = C.CDLL(so)
    for prefix in ("ring_host_", "half_host_"):
        fn = lambda name: getattr(lib, prefix + name)
        fn("create").restype = C.c_void_p
        fn("create").argtypes = [C.c_int, C.c_int]
        fn("destroy").argtypes = [C.c_void_p]
        fn("push").argtypes = [C.c_void_p, C.c_double]
        fn("fetch").restype = C.c_int64
        fn("fetch").argtypes = [C.c_void_p, C.POINTER(C.c_double), C.c_int64]
        fn("pending").restype = C.c_int64
        fn("pending").argtypes = [C.c_void_p]
    return lib


class Ring:
    """A RowRing of ``capacity`` rows of ``width`` doubles.  ``push(tag)`` records the row ``tag + 0.25 * j``
    and returns the index the ring handed out; ``fetch(max_rows)`` returns ``[rows][width]``."""

    prefix = "ring_host_"
    keeps_count = False                # a fetch empties the ring: the next row is 0 again

    def __init__(self, lib, capacity, width):
        self.lib, self.width = lib, width
        self.handle = C.c_void_p(self._fn("create")(capacity, width))

    def _fn(self, name):
        return getattr(self.lib, self.prefix + name)

    def close(self):
        self._fn("destroy")(self.handle)
        self.handle = None

    def push(self, tag):
        return self._fn("push")(self.handle, float(tag))

    def pending(self):
        return self._fn("pending")(self.handle)

    def fetch(self, max_rows):
        out = np.full((max(max_rows, 1), self.width), -7.25)
        n = self._fn("fetch")(self.handle, out.ctypes.data_as(C.POINTER(C.c_double)), max_rows)
        assert 0 <= n <= max(max_rows, 0)
        assert (out[n:] == -7.25).all(), "fetch wrote past the rows it reported"
        return out[:n]


class HalfRing(Ring):
    """A HalfRing of ``capacity`` rows (two halves of ``capacity // 2``) of ``width`` doubles; as ``Ring``."""

    prefix = "half_host_"
    keeps_count = True                 # the index is that of all the rows pushed, modulo the capacity
