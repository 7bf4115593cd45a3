"""TEST-ONLY: build and drive the host harness of the device hooks (hook_host.cpp).

Built by tests/observer_host/common.py from the hook block (codegen.lower_hooks) and csrc/tf_hook.h into
tests/hook_host/_build/hook_<hash>.so.  ``Harness.apply`` runs a program on the planes of one system as the
two kernels do, one launch per run of statements.  The triflow_amd package never loads it.
"""
import ctypes as C
import os

import numpy as np

from tests.observer_host import common
from triflow_amd import codegen
from triflow_amd.hooks import ExpressionHook

HERE = os.path.dirname(os.path.abspath(__file__))
HEADERS = ("tf_args.h", "tf_math.h", "tf_layout.h", "tf_kernels.h", "tf_node.h", "tf_hook.h")


def from_plane(L, plane):
    """One partition-interleaved plane of one system -> [N] natural order (the inverse of common.to_plane)."""
    out = np.empty(L.N)
    for p in range(L.P):
        start = p * L.mbase + min(p, L.rem)
        ln = L.mbase + (p < L.rem)
        out[start:start + ln] = plane[np.arange(ln) * L.Ptot + p]
    return out


class Harness:
    """The program ``statements`` of ``model`` on one system of ``x.size`` nodes in ``P`` chunks."""

    def __init__(self, model, statements, x, pars, periodic, P, parvec_mask=0):
        self.model, self.x, self.pars, self.periodic, self.P, self.mask = model, x, pars, periodic, P, parvec_mask
        self.hook = ExpressionHook(model, statements)
        block, self.spec = self.hook.lowered(x.size, parvec_mask)
        self.lib = common.build(model, block, os.path.join(HERE, "hook_host.cpp"), HEADERS, parvec_mask)
        assert self.lib.hook_host_nhook() == len(statements)
        assert self.lib.hook_host_nconst() == len(self.spec["host_consts"])

    def apply(self, t, fields):
        """The state ``fields`` (dict of [N] arrays) after one application at ``t``: dict of the dependent
        variables."""
        L, planes = common.system_planes(self.model, dict(self.spec, host_consts=[]), self.x, fields, self.pars,
                                         self.periodic, self.P, self.mask)
        pv = [np.asarray(self.pars[k], dtype=float) for k in self.model._pars]
        dx = (self.x[-1] - self.x[0]) / (self.x.size - 1)
        planes[6] = np.array(codegen.eval_host_constants(self.spec, dx, pv, t=t) + [0.0])
        state = planes[0].copy()
        runs = np.array([(codegen.HOOK_KINDS.index(self.hook.layout(L.N)[first].kind), first, count)
                         for first, count in self.spec["runs"]], dtype=np.int32)
        rc = self.lib.hook_host_apply(C.byref(L), common.dptr(state), *[common.dptr(a) for a in planes[1:]],
                                      int(len(runs)), runs.ctypes.data_as(C.POINTER(C.c_int)))
        assert rc == 0
        return {name: from_plane(L, state[k * L.plane:(k + 1) * L.plane])
                for k, name in enumerate(self.model._dep_vars)}
