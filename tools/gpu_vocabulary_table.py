"""Measure the accuracy table of the function vocabulary on the GPU (profiles/r08_vocabulary.txt): per
function case of tests/vocab_cases.py the worst error in ulp against mpmath of the device, of the host
build of the same generated code (glibc) and of NumPy, then the S-scaled errors of the model cases.
The libm bounds of the vocabulary suite (vocab_cases.MEASURED_ULP) are read off this table: re-run it
with a new ROCm release.  usage: python tools/gpu_vocabulary_table.py [output file]"""
import os
import subprocess
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import numpy as np  # noqa: E402

from tests import test_gpu_vocabulary as tg  # noqa: E402
from tests import vocab_cases as vc  # noqa: E402
from triflow_amd import compilers, recorders  # noqa: E402


def main(path):
    recorders.discretise = vc.discretise            # (the SymPy objects of log2 ... expm1: as the suite's fixture)
    out = open(path, "w")

    def say(line=""):
        print(line, flush=True)
        out.write(line + "\n")

    try:
        glibc = subprocess.run(["ldd", "--version"], capture_output=True, text=True).stdout.splitlines()[0]
    except (OSError, IndexError):
        glibc = "unknown"
    say("Accuracy of the function vocabulary of the generated code (codegen._CEmitter), against mpmath at %d bits" % vc.PREC)
    say()
    say("device: %s, flags %s" % (compilers.hipcc_version(), " ".join(compilers.HIPCC_FLAGS)))
    say("glibc:  the host build of the same generated code (g++, tests/record_host); %s" % glibc)
    say("NumPy:  %s, the reference's path.  Argument sets: tests/vocab_cases.py (%d doubles per case)." % (np.__version__, vc.NARG))
    say("Figures: worst |value - exact| in ulp of the exact value.")
    say()
    say("1. Function cases (a recorder with pool=\"sample\" over every node)")
    say()
    say("%-8s %-20s %-6s %-18s %8s %8s %8s   %s" % ("group", "case", "class", "bound key", "device", "glibc", "NumPy",
                                                     "device worst at u ="))
    worst = {}
    for g, (cases, _) in vc.FUNCTION_GROUPS.items():
        for c in cases:
            exact, ref = vc.case_references(g, c)
            got, host = tg.device_row(g, c), vc.host_row(g, c)
            ed, eh, en = vc.ulp_errors(got, exact), vc.ulp_errors(host, exact), vc.ulp_errors(ref, exact)
            say("%-8s %-20s %-6s %-18s %8.3f %8.3f %8.3f   %-24r bytes = host build: %-5s = NumPy: %-5s "
                "not nearest: device %d, host %d"
                % (g, c.name, c.kind, c.fn if c.kind == "libm" else "-", ed.max(), eh.max(), en.max(),
                   float(c.state()["U"][ed.argmax()]), got.tobytes() == host.tobytes(), got.tobytes() == ref.tobytes(),
                   len(vc.not_nearest(got, exact)), len(vc.not_nearest(host, exact))))
            if c.kind == "libm":
                d, h = worst.get(c.fn, (0.0, 0.0))
                worst[c.fn] = (max(d, ed.max()), max(h, eh.max()))
            if c.kind == "divu":
                ones = vc.is_all_ones(c.state()["V"])
                e1 = vc.ulp_errors(got[ones], [e for e, o in zip(exact, ones) if o])
                say("         %s over %d divisors with an all-ones significand: worst %.3f ulp, %d differ from IEEE division"
                    % (c.name, ones.sum(), e1.max(), (got[ones] != ref[ones]).sum()))
    say()
    say("   per bound key (device, glibc) -> vocab_cases.MEASURED_ULP; asserted: ceil(measured) + 1 ulp, cap %d" % vc.LIBM_CAP)
    for fn, (d, h) in worst.items():
        say("   %-12s %.3f %.3f" % (fn, d, h))
    say()
    say("2. Model cases (N = %d): worst |entry - exact| / ulp(S), S = exact sum of |top-level additive terms| of the" % vc.MODEL_N)
    say("   entry; kernel = the F / J sweeps on the device, NumPy = the oracle's lambdified expressions, same inputs")
    say()
    report = []
    for name in sorted(vc.MODEL_CASES):
        for periodic in (True, False):
            for per_node in (False, True):
                vc.check_model_case(name, None, periodic, per_node, report=report)
    for r in report:
        say("   %(case)-32s F: kernel %(F_dev).3f NumPy %(F_numpy).3f   J: kernel %(J_dev).3f NumPy %(J_numpy).3f" % r)
    out.close()


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "r08_vocabulary.txt")
