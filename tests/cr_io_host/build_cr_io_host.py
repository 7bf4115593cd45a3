"""TEST-ONLY: build and run the host harness of the wide memory phases' index mapping (cr_io_host.cpp).

g++ compiles cr_io_host.cpp with csrc/tf_cr_io.h into tests/cr_io_host/_build/cr_io_host_<hash>; ``run``
returns (exit status, output).  The triflow_amd package never loads it.
"""
import hashlib
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(os.path.dirname(HERE)), "triflow_amd", "csrc")
BUILD = os.path.join(HERE, "_build")
SOURCES = (os.path.join(HERE, "cr_io_host.cpp"), os.path.join(CSRC, "tf_cr_io.h"))


def build():
    h = hashlib.sha1()
    for path in SOURCES:
        with open(path, "rb") as f:
            h.update(f.read())
    exe = os.path.join(BUILD, "cr_io_host_%s" % h.hexdigest()[:16])
    if not os.path.exists(exe):
        os.makedirs(BUILD, exist_ok=True)
        cxx = shutil.which("g++") or shutil.which("c++")
        assert cxx, "the harness needs a host C++ compiler"
        tmp = exe + ".%d.tmp" % os.getpid()
        res = subprocess.run([cxx, "-O1", "-std=c++17", "-Wall", "-I", CSRC, SOURCES[0], "-o", tmp],
                             capture_output=True, text=True)
        assert res.returncode == 0, res.stderr[-4000:]
        os.replace(tmp, exe)
    return exe


def run():
    res = subprocess.run([build()], capture_output=True, text=True)
    return res.returncode, res.stdout + res.stderr
