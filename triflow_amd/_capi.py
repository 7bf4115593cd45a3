"""ctypes binding of ``libtriflow_hip.so`` (C ABI in ``include/triflow_hip.h``).

Thin by design: numpy arrays in, numpy arrays out, every non-zero return code
becomes a ``RuntimeError`` carrying ``tf_last_error()``.
"""

import ctypes as C
import os

import numpy as np

c_double_p = C.POINTER(C.c_double)
c_int32_p = C.POINTER(C.c_int32)
c_int64_p = C.POINTER(C.c_int64)


class ModelSpec(C.Structure):
    _fields_ = [("nvar", C.c_int32), ("nh", C.c_int32), ("npar", C.c_int32),
                ("mp", C.c_int32), ("nnz", C.c_int32), ("seg", C.c_int32),
                ("sweep_block", C.c_int32), ("uses_x", C.c_int32),
                ("parvec_mask", C.c_uint32)]


class SolverOpts(C.Structure):
    _fields_ = [("m1", C.c_int32), ("m_upper", C.c_int32), ("nstate", C.c_int32),
                ("refine", C.c_int32), ("device", C.c_int32), ("berr_every", C.c_int32),
                ("reserved", C.c_int32)]


class Scheme(C.Structure):
    _fields_ = [("kind", C.c_int32), ("stages", C.c_int32), ("theta", C.c_double),
                ("alpha", c_double_p), ("gamma", c_double_p), ("b", c_double_p),
                ("hook_after", C.c_int32), ("reserved", C.c_int32)]


#: name -> (restype, argtypes); every symbol declared in include/triflow_hip.h
SIGNATURES = {
    "tf_last_error": (C.c_char_p, []),
    "tf_runtime_info": (C.c_int, [c_int32_p, c_int32_p]),
    "tf_set_device": (C.c_int, [C.c_int32]),
    "tf_model_create": (C.c_int, [C.POINTER(ModelSpec), C.c_void_p, C.c_size_t,
                                  C.POINTER(C.c_void_p)]),
    "tf_model_add_alternate": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint64]),
    "tf_model_destroy": (None, [C.c_void_p]),
    "tf_solver_create": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int32,
                                   C.POINTER(SolverOpts), C.POINTER(C.c_void_p)]),
    "tf_solver_destroy": (None, [C.c_void_p]),
    "tf_solver_describe": (C.c_int, [C.c_void_p, c_int32_p, c_int32_p, C.c_int32, c_int64_p]),
    "tf_set_state": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, c_double_p]),
    "tf_get_state": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, c_double_p]),
    "tf_set_state_flat": (C.c_int, [C.c_void_p, C.c_int32, c_double_p]),
    "tf_get_state_flat": (C.c_int, [C.c_void_p, C.c_int32, c_double_p]),
    "tf_copy_state": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32]),
    "tf_set_helpers": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, c_double_p]),
    "tf_set_param_scalar": (C.c_int, [C.c_void_p, C.c_int32, c_double_p]),
    "tf_set_param_vector": (C.c_int, [C.c_void_p, C.c_int32, c_double_p]),
    "tf_set_dx": (C.c_int, [C.c_void_p, c_double_p]),
    "tf_set_x": (C.c_int, [C.c_void_p, c_double_p]),
    "tf_set_dirichlet": (C.c_int, [C.c_void_p, C.c_int32, c_int32_p, c_int64_p, c_double_p]),
    "tf_set_dirichlet_values": (C.c_int, [C.c_void_p, c_double_p, c_double_p]),
    "tf_poke": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, c_int32_p, c_int64_p, c_double_p]),
    "tf_peek": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, c_int32_p, c_int64_p, c_double_p]),
    "tf_eval": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32]),
    "tf_eval_repeat": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, c_double_p]),
    "tf_get_F": (C.c_int, [C.c_void_p, c_double_p]),
    "tf_get_J": (C.c_int, [C.c_void_p, c_double_p]),
    "tf_set_csc_map": (C.c_int, [C.c_void_p, c_int32_p, C.c_int64]),
    "tf_set_constant_jacobian": (C.c_int, [C.c_void_p, C.c_int32]),
    "tf_get_J_mapped": (C.c_int, [C.c_void_p, c_double_p]),
    "tf_factor": (C.c_int, [C.c_void_p, C.c_double]),
    "tf_solve": (C.c_int, [C.c_void_p, c_double_p, c_double_p]),
    "tf_matvec": (C.c_int, [C.c_void_p, c_double_p, c_double_p]),
    "tf_step_theta": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_double, C.c_double]),
    "tf_step_row": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_double, C.c_int32,
                              c_double_p, c_double_p, c_double_p, c_double_p, C.c_int32,
                              c_double_p]),
    "tf_step_erk": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_double, C.c_int32,
                              c_double_p, c_double_p, c_double_p, C.c_int32, c_double_p]),
    "tf_erk_info": (C.c_int, [C.c_void_p, c_int32_p, c_int64_p, c_int64_p]),
    "tf_step_row_queued": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_double, C.c_int32,
                                     c_double_p, c_double_p, c_double_p, c_double_p, C.c_int32, C.c_int32]),
    "tf_read_err": (C.c_int, [C.c_void_p, C.c_int32, c_double_p]),
    "tf_step_bdf2": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_double]),
    "tf_bdf2_reset": (C.c_int, [C.c_void_p]),
    "tf_step_bdf2_from": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_double]),
    "tf_step_bdf2_owned": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_double, C.c_int64,
                                     C.c_int32]),
    "tf_bdf2_release": (C.c_int, [C.c_void_p, C.c_int64]),
    "tf_diff_norm": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, c_double_p]),
    "tf_step_doubling": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_double,
                                   C.c_int32, C.c_int32, C.POINTER(Scheme), C.c_int32, c_double_p]),
    "tf_backward_error": (C.c_int, [C.c_void_p, c_double_p, c_int32_p]),
    "tf_monitor_error": (C.c_int, [C.c_void_p, c_double_p]),
    "tf_solver_counters": (C.c_int, [C.c_void_p, c_int64_p, c_int64_p, c_int64_p]),
    "tf_jacobian_sweeps": (C.c_int, [C.c_void_p, c_int64_p, c_int64_p]),
    "tf_sync": (C.c_int, [C.c_void_p]),
    "tf_timing_enable": (C.c_int, [C.c_void_p, C.c_int64]),
    "tf_timing_reset": (C.c_int, [C.c_void_p]),
    "tf_timing_get": (C.c_int, [C.c_void_p, C.c_int32, c_double_p, c_int64_p]),
    "tf_debug_stamps": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.c_int32]),
    "tf_solver_kernel_block": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_int32)]),
    "tf_kernel_count": (C.c_int, []),
    "tf_kernel_name": (C.c_char_p, [C.c_int32]),
    "tf_probe_create": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int32, c_int32_p, C.c_int32,
                                  C.c_int32, C.POINTER(C.c_void_p)]),
    "tf_probe_destroy": (None, [C.c_void_p]),
    "tf_probe_set_consts": (C.c_int, [C.c_void_p, c_double_p, C.c_int32]),
    "tf_probe_set_x": (C.c_int, [C.c_void_p, c_double_p]),
    "tf_probe_record": (C.c_int, [C.c_void_p, C.c_int32]),
    "tf_probe_fetch": (C.c_int, [C.c_void_p, c_double_p, C.c_int64, c_int64_p]),
    "tf_probe_pending": (C.c_int, [C.c_void_p, c_int64_p]),
    "tf_record_create": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int32, c_int32_p, C.c_int32,
                                   C.POINTER(C.c_void_p)]),
    "tf_record_destroy": (None, [C.c_void_p]),
    "tf_record_set_consts": (C.c_int, [C.c_void_p, c_double_p, C.c_int32]),
    "tf_record_set_x": (C.c_int, [C.c_void_p, c_double_p]),
    "tf_record_record": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32]),
    "tf_record_fetch": (C.c_int, [C.c_void_p, C.c_int32, c_double_p, C.c_int64, c_int64_p]),
    "tf_record_pending": (C.c_int, [C.c_void_p, C.c_int32, c_int64_p]),
    "tf_stat_create": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int32, c_int32_p, C.c_int32,
                                 C.POINTER(C.c_void_p)]),
    "tf_stat_destroy": (None, [C.c_void_p]),
    "tf_stat_set_consts": (C.c_int, [C.c_void_p, c_double_p, C.c_int32]),
    "tf_stat_set_x": (C.c_int, [C.c_void_p, c_double_p]),
    "tf_stat_update": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int64, C.c_double]),
    "tf_stat_planes_of": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_int32)]),
    "tf_stat_fetch": (C.c_int, [C.c_void_p, C.c_int32, c_double_p]),
    "tf_stat_load": (C.c_int, [C.c_void_p, C.c_int32, c_double_p]),
    "tf_spectrum_create": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int32, c_int32_p, C.c_int32,
                                     C.POINTER(C.c_void_p)]),
    "tf_spectrum_destroy": (None, [C.c_void_p]),
    "tf_spectrum_set_consts": (C.c_int, [C.c_void_p, c_double_p, C.c_int32]),
    "tf_spectrum_set_x": (C.c_int, [C.c_void_p, c_double_p]),
    "tf_spectrum_set_modes": (C.c_int, [C.c_void_p, C.c_int32, c_int32_p, C.c_int32]),
    "tf_spectrum_record": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32]),
    "tf_spectrum_fetch": (C.c_int, [C.c_void_p, C.c_int32, c_double_p, C.c_int64, c_int64_p]),
    "tf_spectrum_pending": (C.c_int, [C.c_void_p, C.c_int32, c_int64_p]),
    "tf_extrema_create": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int32, c_int32_p, c_double_p, C.c_int32,
                                    C.POINTER(C.c_void_p)]),
    "tf_extrema_destroy": (None, [C.c_void_p]),
    "tf_extrema_set_consts": (C.c_int, [C.c_void_p, c_double_p, C.c_int32]),
    "tf_extrema_set_x": (C.c_int, [C.c_void_p, c_double_p]),
    "tf_extrema_record": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32]),
    "tf_extrema_fetch": (C.c_int, [C.c_void_p, C.c_int32, c_double_p, C.c_int64, c_int64_p]),
    "tf_extrema_pending": (C.c_int, [C.c_void_p, C.c_int32, c_int64_p]),
    "tf_histogram_create": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int32, c_int32_p, C.c_int32,
                                      C.POINTER(C.c_void_p)]),
    "tf_histogram_destroy": (None, [C.c_void_p]),
    "tf_histogram_set_consts": (C.c_int, [C.c_void_p, c_double_p, C.c_int32]),
    "tf_histogram_set_x": (C.c_int, [C.c_void_p, c_double_p]),
    "tf_histogram_set_edges": (C.c_int, [C.c_void_p, C.c_int32, c_double_p, C.c_int32]),
    "tf_histogram_record": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32]),
    "tf_histogram_fetch": (C.c_int, [C.c_void_p, C.c_int32, c_double_p, C.c_int64, c_int64_p]),
    "tf_histogram_pending": (C.c_int, [C.c_void_p, C.c_int32, c_int64_p]),
    "tf_hook_create": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int32, c_int32_p, C.c_int32,
                                 C.POINTER(C.c_void_p)]),
    "tf_hook_destroy": (None, [C.c_void_p]),
    "tf_hook_set_x": (C.c_int, [C.c_void_p, c_double_p]),
    "tf_hook_set_consts": (C.c_int, [C.c_void_p, c_double_p, c_double_p, C.c_double, C.c_double]),
    "tf_hook_attach": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32]),
    "tf_hook_apply": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32]),
}


def _dptr(arr):
    return arr.ctypes.data_as(c_double_p)


def _f64(a, shape=None):
    out = np.ascontiguousarray(a, dtype=np.float64)
    if shape is not None and out.shape != tuple(shape):
        raise ValueError("expected array of shape %r, got %r" % (tuple(shape), out.shape))
    return out


class Library:
    """A loaded ``libtriflow_hip.so`` with typed entry points."""

    def __init__(self, path):
        if not os.path.exists(path):
            raise RuntimeError(
                "HIP runtime library %s is missing -- build it with "
                "`python -c 'import __graft_entry__ as g; g.build()'` "
                "(there is no CPU fallback)" % path)
        self.path = path
        self.dll = C.CDLL(path)
        for name, (restype, argtypes) in SIGNATURES.items():
            fn = getattr(self.dll, name)
            fn.restype = restype
            fn.argtypes = argtypes

    def call(self, name, *args):
        rc = getattr(self.dll, name)(*args)
        if rc != 0:
            raise RuntimeError("%s: %s" % (name, self.dll.tf_last_error().decode()))

    def runtime_info(self):
        dev, cnt = C.c_int32(0), C.c_int32(0)
        self.call("tf_runtime_info", C.byref(dev), C.byref(cnt))
        return bool(dev.value), cnt.value

    def set_device(self, ordinal):
        self.call("tf_set_device", int(ordinal))

    def kernel_names(self):
        return [self.dll.tf_kernel_name(k).decode() for k in range(self.dll.tf_kernel_count())]


class DeviceModel:
    """``tf_model``: a loaded per-model code object."""

    def __init__(self, lib, spec, code, alt_code=None, alt_kernels=()):
        self.lib = lib
        self.spec = dict(spec)
        cs = ModelSpec(spec["nvar"], spec["nh"], spec["npar"], spec["mp"], spec["nnz"],
                       spec["seg"], spec["sweep_block"], spec["uses_x"], spec["parvec_mask"])
        self._code = C.create_string_buffer(code, len(code)) if code else None
        handle = C.c_void_p()
        lib.call("tf_model_create", C.byref(cs),
                 C.cast(self._code, C.c_void_p) if self._code is not None else None,
                 len(code) if code else 0, C.byref(handle))
        self.handle = handle
        self._alt = None
        if alt_code and alt_kernels:
            names = lib.kernel_names()
            mask = 0
            for k in alt_kernels:
                mask |= 1 << names.index(k)
            self._alt = C.create_string_buffer(alt_code, len(alt_code))
            lib.call("tf_model_add_alternate", handle, C.cast(self._alt, C.c_void_p), len(alt_code), mask)

    def close(self):
        if self.handle:
            self.lib.dll.tf_model_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DeviceSolver:
    """``tf_solver``: resident state + kernels for ``nsys`` systems of ``N`` nodes."""

    def __init__(self, model, N, nsys=1, periodic=False, m1=0, m_upper=0, nstate=0,
                 refine=-1, device=-1, berr_every=0):
        self.model = model
        self.lib = model.lib
        self.N, self.nsys, self.periodic = int(N), int(nsys), bool(periodic)
        self.nvar, self.nh = model.spec["nvar"], model.spec["nh"]
        self.npar, self.nnz = model.spec["npar"], model.spec["nnz"]
        m1 = m1 or int(os.environ.get("TRIFLOW_M1", "0"))
        m_upper = m_upper or int(os.environ.get("TRIFLOW_M_UPPER", "0"))
        opts = SolverOpts(m1, m_upper, nstate, refine, device, berr_every, 0)
        handle = C.c_void_p()
        self.lib.call("tf_solver_create", model.handle, self.N, self.nsys,
                      int(self.periodic), C.byref(opts), C.byref(handle))
        self.handle = handle
        self.nstate = nstate if nstate > 0 else 3
        # constant-coefficient linear model: the factorisation of a step is kept while c and the
        # parameters are unchanged (tf_set_constant_jacobian)
        ju = model.spec.get("j_uniform") or []
        self.constant_jacobian = bool(ju) and all(ju) and os.environ.get("TRIFLOW_REUSE_FACTOR", "1") != "0"
        if self.constant_jacobian:
            self.lib.call("tf_set_constant_jacobian", self.handle, 1)

    def close(self):
        if self.handle:
            self.lib.dll.tf_solver_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def describe(self):
        nl, nbytes = C.c_int32(0), C.c_int64(0)
        chunks = (C.c_int32 * 32)()
        self.lib.call("tf_solver_describe", self.handle, C.byref(nl), chunks, 32, C.byref(nbytes))
        return dict(levels=nl.value, chunks=list(chunks[:nl.value]), device_bytes=nbytes.value)

    # ------------------------------------------------------------------ inputs
    def set_state(self, slot, arrays, first=0):
        """``arrays``: [nvars][nsys][N] (or [nvars][N] when nsys == 1)."""
        a = _f64(arrays).reshape(-1, self.nsys, self.N)
        self.lib.call("tf_set_state", self.handle, slot, first, a.shape[0], _dptr(a))

    def get_state(self, slot, first=0, nvars=None):
        nvars = self.nvar - first if nvars is None else nvars
        out = np.empty((nvars, self.nsys, self.N))
        self.lib.call("tf_get_state", self.handle, slot, first, nvars, _dptr(out))
        return out

    def set_state_flat(self, slot, uflat):
        a = _f64(uflat).reshape(self.nsys, self.N * self.nvar)
        self.lib.call("tf_set_state_flat", self.handle, slot, _dptr(a))

    def get_state_flat(self, slot):
        out = np.empty((self.nsys, self.N * self.nvar))
        self.lib.call("tf_get_state_flat", self.handle, slot, _dptr(out))
        return out

    def copy_state(self, src, dst):
        self.lib.call("tf_copy_state", self.handle, src, dst)

    def set_helpers(self, arrays, first=0):
        a = _f64(arrays).reshape(-1, self.nsys, self.N)
        self.lib.call("tf_set_helpers", self.handle, first, a.shape[0], _dptr(a))

    def set_param(self, k, value):
        """Scalar per system, or [nsys][N] per-node values when the model was
        compiled with parameter ``k`` as a vector."""
        if (self.model.spec["parvec_mask"] >> k) & 1:
            a = _f64(np.broadcast_to(np.asarray(value, dtype=float), (self.nsys, self.N)))
            self.lib.call("tf_set_param_vector", self.handle, k, _dptr(a))
        else:
            a = _f64(np.broadcast_to(np.asarray(value, dtype=float), (self.nsys,)))
            self.lib.call("tf_set_param_scalar", self.handle, k, _dptr(a))

    def set_dx(self, dx):
        a = _f64(np.broadcast_to(np.asarray(dx, dtype=float), (self.nsys,)))
        self.lib.call("tf_set_dx", self.handle, _dptr(a))

    def set_x(self, x):
        a = _f64(np.broadcast_to(np.asarray(x, dtype=float), (self.nsys, self.N)))
        self.lib.call("tf_set_x", self.handle, _dptr(a))

    def set_dirichlet(self, entries):
        """``entries``: iterable of (variable index, node index, value)."""
        entries = list(entries)
        n = len(entries)
        var = np.array([e[0] for e in entries], dtype=np.int32)
        node = np.array([e[1] for e in entries], dtype=np.int64)
        val = np.array([e[2] for e in entries], dtype=np.float64)
        self.lib.call("tf_set_dirichlet", self.handle, n,
                      var.ctypes.data_as(c_int32_p), node.ctypes.data_as(c_int64_p), _dptr(val))

    def poke(self, slot, entries):
        """Point writes ``(variable index, node index, value)`` into a resident slot."""
        entries = list(entries)
        if not entries:
            return
        var = np.array([e[0] for e in entries], dtype=np.int32)
        node = np.array([e[1] for e in entries], dtype=np.int64)
        val = np.array([e[2] for e in entries], dtype=np.float64)
        self.lib.call("tf_poke", self.handle, slot, len(entries),
                      var.ctypes.data_as(c_int32_p), node.ctypes.data_as(c_int64_p), _dptr(val))

    def peek(self, slot, var, node):
        """Value of one node of a resident slot (per system)."""
        v = np.array([var], dtype=np.int32)
        n = np.array([node], dtype=np.int64)
        out = np.empty((1, self.nsys))
        self.lib.call("tf_peek", self.handle, slot, 1, v.ctypes.data_as(c_int32_p),
                      n.ctypes.data_as(c_int64_p), _dptr(out))
        return out[0]

    def set_dirichlet_values(self, before=None, after=None):
        b = _f64(before) if before is not None else None
        a = _f64(after) if after is not None else None
        self.lib.call("tf_set_dirichlet_values", self.handle,
                      _dptr(b) if b is not None else None, _dptr(a) if a is not None else None)

    # ----------------------------------------------------------------- seam #1
    def eval(self, slot=0, with_j=False):
        self.lib.call("tf_eval", self.handle, slot, int(with_j))

    def eval_repeat(self, slot=0, with_j=True, reps=20):
        """Mean duration (ms) of ``reps`` back-to-back sweeps (two HIP events)."""
        ms = C.c_double(0.0)
        self.lib.call("tf_eval_repeat", self.handle, slot, int(with_j), reps, C.byref(ms))
        return ms.value / reps

    def get_F(self):
        out = np.empty((self.nsys, self.N * self.nvar))
        self.lib.call("tf_get_F", self.handle, _dptr(out))
        return out

    def get_J(self):
        out = np.empty((self.nsys, self.N, max(self.nnz, 1)))
        self.lib.call("tf_get_J", self.handle, _dptr(out))
        return out[:, :, :self.nnz]

    def set_csc_map(self, index_list):
        """Value-table index (node * nnz + k) of every entry ``get_J_mapped`` is to return."""
        m = np.ascontiguousarray(index_list, dtype=np.int32)
        self.lib.call("tf_set_csc_map", self.handle, m.ctypes.data_as(c_int32_p), m.size)
        self._csc_n = m.size

    def get_J_mapped(self):
        out = np.empty(self._csc_n)
        self.lib.call("tf_get_J_mapped", self.handle, _dptr(out))
        return out

    # ----------------------------------------------------------------- seam #3
    def factor(self, c):
        self.lib.call("tf_factor", self.handle, float(c))

    def solve(self, rhs_flat):
        rhs = _f64(rhs_flat).reshape(self.nsys, self.N * self.nvar)
        out = np.empty_like(rhs)
        self.lib.call("tf_solve", self.handle, _dptr(rhs), _dptr(out))
        return out

    def matvec(self, v_flat):
        v = _f64(v_flat).reshape(self.nsys, self.N * self.nvar)
        out = np.empty_like(v)
        self.lib.call("tf_matvec", self.handle, _dptr(v), _dptr(out))
        return out

    # ----------------------------------------------------------------- seam #2
    def step_theta(self, src, dst, dt, theta=1.0):
        self.lib.call("tf_step_theta", self.handle, src, dst, float(dt), float(theta))

    def step_row(self, src, dst, dt, alpha, gamma, b, b_pred=None, hook_after=False,
                 want_err=True):
        alpha, gamma = _f64(alpha), _f64(gamma)
        b = _f64(b)
        s = b.size
        bp = _f64(b_pred) if b_pred is not None else None
        err = C.c_double(0.0)
        self.lib.call("tf_step_row", self.handle, src, dst, float(dt), s, _dptr(alpha),
                      _dptr(gamma), _dptr(b), _dptr(bp) if bp is not None else None,
                      int(hook_after), C.byref(err) if want_err else None)
        return np.float64(err.value) if (want_err and bp is not None) else None

    def step_erk(self, src, dst, dt, a, b, d=None, hook_after=False, want_err=True):
        """One explicit Runge-Kutta step (``tf_step_erk``); ``d = b - b_err`` or None.  Returns the
        error estimate ``max |sum_i d_i k_i|`` when ``d`` is given and wanted, else None."""
        a, b = _f64(a), _f64(b)
        s = b.size
        if a.size != s * s:
            raise ValueError("step_erk: a is [s][s], b is [s]")
        dd = _f64(d) if d is not None else None
        if dd is not None and dd.size != s:
            raise ValueError("step_erk: d is [s]")
        err = C.c_double(0.0)
        self.lib.call("tf_step_erk", self.handle, src, dst, float(dt), s, _dptr(a), _dptr(b),
                      _dptr(dd) if dd is not None else None, int(hook_after),
                      C.byref(err) if want_err else None)
        return np.float64(err.value) if (want_err and dd is not None) else None

    def erk_info(self):
        """dict(fused, steps, fused_steps): the form of this solver's explicit steps and how many it took."""
        f, n, nf = C.c_int32(0), C.c_int64(0), C.c_int64(0)
        self.lib.call("tf_erk_info", self.handle, C.byref(f), C.byref(n), C.byref(nf))
        return dict(fused=bool(f.value), steps=n.value, fused_steps=nf.value)

    def step_row_queued(self, src, dst, dt, alpha, gamma, b, b_pred, hook_after=False, err_slot=1):
        """The same step; its embedded error estimate stays on the device (reduction slot ``err_slot``)
        until :meth:`read_err` fetches it."""
        alpha, gamma, b, bp = _f64(alpha), _f64(gamma), _f64(b), _f64(b_pred)
        self.lib.call("tf_step_row_queued", self.handle, src, dst, float(dt), b.size, _dptr(alpha),
                      _dptr(gamma), _dptr(b), _dptr(bp), int(hook_after), int(err_slot))

    def read_err(self, err_slot):
        err = C.c_double(0.0)
        self.lib.call("tf_read_err", self.handle, int(err_slot), C.byref(err))
        return np.float64(err.value)

    def step_bdf2(self, src, dst, dt, owner=0, continuing=True):
        """``owner`` 0: the solver's own history (a caller that owns the solver); otherwise the
        history buffer of one scheme instance (``tf_step_bdf2_owned``)."""
        if owner:
            self.lib.call("tf_step_bdf2_owned", self.handle, src, dst, float(dt), int(owner),
                          int(bool(continuing)))
        else:
            self.lib.call("tf_step_bdf2", self.handle, src, dst, float(dt))

    def step_bdf2_from(self, src, dst, prev, dt):
        """BDF-2 step whose history U_{n-1} is in state slot ``prev`` (-1: none, backward-Euler form)."""
        self.lib.call("tf_step_bdf2_from", self.handle, src, dst, int(prev), float(dt))

    def bdf2_release(self, owner):
        if self.handle:
            self.lib.call("tf_bdf2_release", self.handle, int(owner))

    def bdf2_reset(self):
        self.lib.call("tf_bdf2_reset", self.handle)

    def step_doubling(self, src, dst, tmp, coarse, dt, m, desc, ord=2, nfine=10):
        """One step-doubling trial (``tf_step_doubling``); ``desc``: dict(kind="theta", theta=..)
        or dict(kind="row", alpha=.., gamma=.., b=.., hook_after=..).  Returns err per system."""
        keep = []
        if desc["kind"] == "theta":
            sch = Scheme(0, 0, float(desc["theta"]), None, None, None, 0, 0)
        else:
            arrs = [_f64(desc[k]) for k in ("alpha", "gamma", "b")]
            keep.extend(arrs)
            sch = Scheme(1, arrs[2].size, 0.0, _dptr(arrs[0]), _dptr(arrs[1]), _dptr(arrs[2]),
                         int(bool(desc.get("hook_after", True))), 0)
        err = np.empty(self.nsys)
        self.lib.call("tf_step_doubling", self.handle, src, dst, tmp, coarse, float(dt), int(m),
                      int(nfine), C.byref(sch), 0 if ord in (0, np.inf, "inf") else int(ord), _dptr(err))
        return err

    def diff_norms(self, slot_a, slot_b, ord=2):
        """||state[a] - state[b]|| per system and dependent variable, [nsys][nvar]."""
        out = np.empty((self.nsys, self.nvar))
        self.lib.call("tf_diff_norm", self.handle, slot_a, slot_b,
                      0 if ord in (0, np.inf, "inf") else int(ord), _dptr(out))
        return out

    def backward_error(self):
        """(componentwise backward error of the checked solve, refinement active?)"""
        om, flag = C.c_double(0.0), C.c_int32(0)
        self.lib.call("tf_backward_error", self.handle, C.byref(om), C.byref(flag))
        return om.value, bool(flag.value)

    def counters(self):
        """dict(factorisations, checks, replans) since the solver was created."""
        f, c, r = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        self.lib.call("tf_solver_counters", self.handle, C.byref(f), C.byref(c), C.byref(r))
        return dict(factorisations=f.value, checks=c.value, replans=r.value)

    def jacobian_sweeps(self):
        """dict(full, lean): F+J sweeps that wrote every plane of the value table / that left the
        node-independent planes alone (written once per upload of a parameter or dx)."""
        f, n = C.c_int64(0), C.c_int64(0)
        self.lib.call("tf_jacobian_sweeps", self.handle, C.byref(f), C.byref(n))
        return dict(full=f.value, lean=n.value)

    def kernel_block(self, name):
        """Workgroup size the kernel ``name`` of the model's code object was built for."""
        b = C.c_int32(0)
        self.lib.call("tf_solver_kernel_block", self.handle, self.lib.kernel_names().index(name), C.byref(b))
        return b.value

    def monitor_error(self):
        """Worst backward error seen by the in-pass monitor of the Rosenbrock steps since the last
        synchronising call."""
        w = C.c_double(0.0)
        self.lib.call("tf_monitor_error", self.handle, C.byref(w))
        return w.value

    def sync(self):
        self.lib.call("tf_sync", self.handle)
        if not getattr(self, "_warned_replan", False) and self.counters()["replans"]:
            import warnings
            self._warned_replan = True
            warnings.warn("banded solver: the default partition lost accuracy on this matrix and the "
                          "factorisations go through the rescue plan (8 x longer chunks, every solve "
                          "checked): several times slower; see DESIGN.md section 4.5", RuntimeWarning,
                          stacklevel=2)

    def debug_stamps(self, levels=8):
        """[levels][64] uint64 stamps of a -DTF_STAMPS kernel build (first call: switch on)."""
        out = np.zeros((levels, 64), dtype=np.uint64)
        self.lib.call("tf_debug_stamps", self.handle, out.ctypes.data_as(C.POINTER(C.c_uint64)), levels)
        return out

    # ------------------------------------------------------------- measurement
    def timing(self, on=True, kernels=None):
        """Time every launch (``on=True``), none, or only the named ``kernels``."""
        if kernels is not None:
            names = self.lib.kernel_names()
            mask = 0
            for k in kernels:
                mask |= 1 << names.index(k)
        else:
            mask = -1 if on else 0
        self.lib.call("tf_timing_enable", self.handle, mask)

    def timing_reset(self):
        self.lib.call("tf_timing_reset", self.handle)

    def timing_report(self):
        """{kernel name: (total ms, launches)} for kernels launched since reset."""
        out = {}
        for k, name in enumerate(self.lib.kernel_names()):
            ms, n = C.c_double(0.0), C.c_int64(0)
            self.lib.call("tf_timing_get", self.handle, k, C.byref(ms), C.byref(n))
            if n.value:
                out[name] = (ms.value, n.value)
        return out


class _DeviceObserver:
    """What ``tf_probe``, ``tf_record``, ``tf_stat``, ``tf_spectrum``, ``tf_extrema`` and ``tf_histogram`` share: a code object of expressions bound to one solver, the
    x plane and the host constants of the expressions.  ``_prefix``: of the C entry points, ``_noun``:
    what the error message calls the set."""

    _prefix = _noun = None

    def _create(self, solver, code, nconst, *args):
        """``<prefix>_create(solver, code, size, *args, &handle)``"""
        self.solver, self.lib = solver, solver.lib
        self.nconst = int(nconst)
        self._code = C.create_string_buffer(code, len(code))
        handle = C.c_void_p()
        self.lib.call(self._prefix + "_create", solver.handle, C.cast(self._code, C.c_void_p), len(code),
                      *args, C.byref(handle))
        self.handle = handle

    def close(self):
        if self.handle:
            getattr(self.lib.dll, self._prefix + "_destroy")(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check_open(self):
        # (the handle reads its solver's layout, stream and planes: not after the solver is gone)
        if not self.solver.handle:
            raise RuntimeError("the solver of this %s set was closed (rows not fetched before are lost)" % self._noun)

    def _call(self, name, *args):
        self._check_open()
        self.lib.call("%s_%s" % (self._prefix, name), self.handle, *args)

    def set_consts(self, values):
        """``values``: [nsys][nconst] host constants of the expressions."""
        self._check_open()
        v = _f64(values).reshape(self.solver.nsys, self.nconst)
        self._call("set_consts", _dptr(v) if v.size else None, self.nconst)

    def set_x(self, x):
        self._check_open()
        a = _f64(np.broadcast_to(np.asarray(x, dtype=float), (self.solver.nsys, self.solver.N)))
        self._call("set_x", _dptr(a))

    def _pending(self, *which):
        n = C.c_int64(0)
        self._call("pending", *which, C.byref(n))
        return n.value

    def _fetch(self, ncols, *which):
        """Every row recorded since the last fetch, ``[rows][nsys][ncols]``."""
        n = self._pending(*which)
        out = np.empty((n, self.solver.nsys, ncols))
        got = C.c_int64(0)
        self._call("fetch", *which, _dptr(out), n, C.byref(got))
        return out[:got.value]


class DeviceProbe(_DeviceObserver):
    """``tf_probe``: the probe kernels of one probe set bound to one solver, and their ring."""

    _prefix, _noun = "tf_probe", "probe"

    def __init__(self, solver, code, kinds, nconst, capacity=1024):
        self.nprobe, self.capacity = len(kinds), int(capacity)
        k = np.ascontiguousarray(kinds, dtype=np.int32)
        self._create(solver, code, nconst, self.nprobe, k.ctypes.data_as(c_int32_p), int(nconst), self.capacity)

    def record(self, slot):
        self._call("record", int(slot))

    def pending(self):
        return self._pending()

    def fetch(self):
        """Every row recorded since the last fetch, ``[rows][nsys][nprobe]`` (waits for the stream)."""
        return self._fetch(self.nprobe)


class _DeviceRows(_DeviceObserver):
    """What ``tf_record``, ``tf_spectrum``, ``tf_extrema`` and ``tf_histogram`` share besides: a ring of rows
    per item ``which`` of the set.  A subclass shapes the rows of ``_fetch_rows`` in its ``fetch``."""

    fetched = 0                                  # doubles that came to the host through fetch

    def record(self, which, slot):
        self._call("record", int(which), int(slot))

    def pending(self, which):
        return self._pending(int(which))

    def _fetch_rows(self, which, ncols):
        """Every row of item ``which`` recorded since its last fetch, ``[rows][nsys][ncols]`` doubles
        (waits for the stream)."""
        raw = self._fetch(ncols, int(which))
        self.fetched += raw.size
        return raw


class DeviceRecord(_DeviceRows):
    """``tf_record``: the record kernel of one recorder set bound to one solver, and the rings."""

    _prefix, _noun = "tf_record", "recorder"

    def __init__(self, solver, code, geometry, nconst):
        """``geometry``: per recorder ``(expression, pool, start, stop, step, rows of the ring)``."""
        g = np.ascontiguousarray(geometry, dtype=np.int32).reshape(-1, 6)
        self.ncols = [-(-(int(r[3]) - int(r[2])) // int(r[4])) for r in g]
        self._create(solver, code, nconst, len(g), g.ctypes.data_as(c_int32_p), int(nconst))

    def fetch(self, which):
        """Every row of recorder ``which`` recorded since its last fetch, ``[rows][nsys][ncols]``."""
        return self._fetch_rows(which, self.ncols[which])


class DeviceStat(_DeviceObserver):
    """``tf_stat``: the statistic kernel of one statistic set bound to one solver, and the accumulators."""

    _prefix, _noun = "tf_stat", "statistic"

    def __init__(self, solver, code, geometry, nconst):
        """``geometry``: per statistic ``(expression, kind)``; ``kind``: index into
        ``statistics.STATISTIC_KINDS``."""
        g = np.ascontiguousarray(geometry, dtype=np.int32).reshape(-1, 2)
        self._create(solver, code, nconst, len(g), g.ctypes.data_as(c_int32_p), int(nconst))
        self.planes = []                         # per statistic, as the library sized them (tf_stat_planes)
        for k in range(len(g)):
            n = C.c_int32(0)
            self._call("planes_of", k, C.byref(n))
            self.planes.append(n.value)

    def update(self, which, slot, k, t):
        """Fold state ``slot`` into statistic ``which`` as sample ``k`` (1: the first) taken at ``t``."""
        self._call("update", int(which), int(slot), int(k), float(t))

    def fetch(self, which):
        """The accumulators of statistic ``which``, ``[planes][nsys][N]`` (waits for the stream)."""
        out = np.empty((self.planes[which], self.solver.nsys, self.solver.N))
        self._call("fetch", int(which), _dptr(out))
        return out

    def load(self, which, planes):
        """The inverse of ``fetch``."""
        a = _f64(planes, (self.planes[which], self.solver.nsys, self.solver.N))
        self._call("load", int(which), _dptr(a))


class DeviceSpectrum(_DeviceRows):
    """``tf_spectrum``: the spectrum kernels of one spectrum set bound to one solver, the modes and the
    rings."""

    _prefix, _noun = "tf_spectrum", "spectrum"

    def __init__(self, solver, code, geometry, modes, nconst):
        """``geometry``: per spectrum ``(expression, number of modes, rows of the ring)``; ``modes``: per
        spectrum, its modes (uploaded here: they are data of the handle, not of the code object)."""
        g = np.ascontiguousarray(geometry, dtype=np.int32).reshape(-1, 3)
        self.nmodes = [int(r[1]) for r in g]
        self._create(solver, code, nconst, len(g), g.ctypes.data_as(c_int32_p), int(nconst))
        for k, m in enumerate(modes):
            m = np.ascontiguousarray(m, dtype=np.int32)
            self._call("set_modes", k, m.ctypes.data_as(c_int32_p), int(m.size))

    def fetch(self, which):
        """Every row of spectrum ``which`` recorded since its last fetch, ``[rows][nsys][nmodes]``
        complex128 (waits for the stream)."""
        return np.ascontiguousarray(self._fetch_rows(which, 2 * self.nmodes[which])).view(np.complex128)


class DeviceExtrema(_DeviceRows):
    """``tf_extrema``: the extrema kernels of one extrema set bound to one solver, and the rings."""

    _prefix, _noun = "tf_extrema", "extrema"

    def __init__(self, solver, code, geometry, thresholds, nconst):
        """``geometry``: per observer ``(expression, kind, max_count, rows of the ring or 0 for the
        default)``; ``thresholds``: per observer, -inf (max) / +inf (min) for none."""
        g = np.ascontiguousarray(geometry, dtype=np.int32).reshape(-1, 4)
        th = _f64(thresholds).reshape(len(g))
        self.max_count = [int(r[2]) for r in g]
        self._create(solver, code, nconst, len(g), g.ctypes.data_as(c_int32_p), _dptr(th), int(nconst))

    def fetch(self, which):
        """Every row of observer ``which`` recorded since its last fetch, ``[rows][nsys][1 + 4 * max_count]``:
        the count, then ``(g, v[g-1], v[g], v[g+1])`` per entry (waits for the stream)."""
        return self._fetch_rows(which, 1 + 4 * self.max_count[which])


class DeviceHistogram(_DeviceRows):
    """``tf_histogram``: the histogram kernels of one histogram set bound to one solver, the edges and the
    rings."""

    _prefix, _noun = "tf_histogram", "histogram"

    def __init__(self, solver, code, geometry, edges, nconst):
        """``geometry``: per histogram ``(expression, number of bins, rows of the ring, start, stop, step)``;
        ``edges``: per histogram, its ``nbins + 1`` edges (uploaded here: they are data of the handle, not
        of the code object)."""
        g = np.ascontiguousarray(geometry, dtype=np.int32).reshape(-1, 6)
        self.nbins = [int(r[1]) for r in g]
        self._create(solver, code, nconst, len(g), g.ctypes.data_as(c_int32_p), int(nconst))
        for k, e in enumerate(edges):
            e = _f64(e)
            self._call("set_edges", k, _dptr(e), int(e.size))

    def fetch(self, which):
        """Every row of histogram ``which`` recorded since its last fetch, ``[rows][nsys][nbins + 3]``
        int64: the bins, then below, above and NaN (waits for the stream)."""
        return self._fetch_rows(which, self.nbins[which] + 3).astype(np.int64)


class DeviceHook(_DeviceObserver):
    """``tf_hook``: the kernels of one hook program (``hooks.ExpressionHook``) bound to one solver, and the two
    sets of its host constants.  Unlike the observers it writes the state: attached, the solver's step
    functions run it where they apply the Dirichlet list."""

    _prefix, _noun = "tf_hook", "hook"

    def __init__(self, solver, code, geometry, nconst):
        """``geometry``: per statement ``(kind, variable, node, 0, 0)`` or ``(kind, variable, start, stop,
        step)`` (``codegen.HookStatement.geometry``)."""
        g = np.ascontiguousarray(geometry, dtype=np.int32).reshape(-1, 5)
        self.attached = False
        self._create(solver, code, nconst, len(g), g.ctypes.data_as(c_int32_p), int(nconst))

    def set_consts(self, before, after, t_before, t_after):
        """``before`` / ``after``: [nsys][nconst] host constants for the call before the step / after it."""
        self._check_open()
        b = _f64(before).reshape(self.solver.nsys, self.nconst)
        a = _f64(after).reshape(self.solver.nsys, self.nconst)
        self._call("set_consts", _dptr(b) if b.size else None, _dptr(a) if a.size else None,
                   float(t_before), float(t_after))

    def attach(self, on=True, idempotent=False):
        self._call("attach", int(bool(on)), int(bool(idempotent)))
        self.attached = bool(on)

    def apply(self, src, dst):
        """One application outside a step, with the ``before`` constants: slot ``src`` -> slot ``dst``."""
        self._call("apply", int(src), int(dst))

    def close(self):
        if self.handle and self.attached and self.solver.handle:
            self.attach(False)                      # (the solver's captured steps hold the program's launches)
        super().close()
