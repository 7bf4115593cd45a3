// The partition-interleaved layout of a solver level (TfLayout, tf_args.h): where node i of chunk p of
// system e lives in a plane, and which element stands for a node beyond the ends of a chunk.  What the
// solver kernels (tf_kernels.h) and the node core of the device observers (tf_node.h) share; it follows
// the generated model constants (TF_NVAR, TF_NH, TF_MP) in a translation unit.
#pragma once
#include "tf_args.h"

#ifndef TF_DEVICE
#error "define TF_DEVICE (e.g. __device__ __forceinline__) before including tf_layout.h"
#endif

#define TF_W (2 * TF_MP + 1)
#define TF_NF (TF_NVAR + TF_NH)

TF_DEVICE int tf_len(const TfLayout& L, int p) { return L.mbase + (p < L.rem ? 1 : 0); }
TF_DEVICE int tf_start(const TfLayout& L, int p) { return p * L.mbase + (p < L.rem ? p : L.rem); }
TF_DEVICE int64_t tf_idx(const TfLayout& L, int pg, int i) { return (int64_t)i * L.Ptot + pg; }
// Element of plane k at byte offset off8 = 8 * tf_idx(...): the plane's base stays in scalar
// registers and the lane offset is 32 bits wide (global_load/store with saddr: no 64-bit address
// arithmetic per access).  A plane is smaller than 4 GB (tf_solver_create checks).
TF_DEVICE unsigned tf_off8(const TfLayout& L, int pg, int i) { return (unsigned)tf_idx(L, pg, i) * 8u; }
TF_DEVICE double tf_ldp(const double* base, int64_t k, int64_t plane, unsigned off8) {
    return *(const double*)((const char*)(base + k * plane) + off8);
}
TF_DEVICE void tf_stp(double* base, int64_t k, int64_t plane, unsigned off8, double v) {
    *(double*)((char*)(base + k * plane) + off8) = v;
}

// element of the node `d` places after node i of chunk (e, p); wraps or clamps
// at the ends of the system exactly like the ghost cells of
// triflow/core/compilers.py:257-264.  Needs |d| <= mbase.
TF_DEVICE int64_t tf_nbr(const TfLayout& L, int e, int p, int len, int i, int d) {
    int ii = i + d;
    int pp = p;
    if (ii < 0) {
        if (p > 0) { pp = p - 1; ii += tf_len(L, pp); }
        else if (L.periodic) { pp = L.P - 1; ii += tf_len(L, pp); }
        else ii = 0;
    } else if (ii >= len) {
        if (p < L.P - 1) { pp = p + 1; ii -= len; }
        else if (L.periodic) { pp = 0; ii -= len; }
        else ii = len - 1;
    }
    return tf_idx(L, e * L.P + pp, ii);
}

// node index -> (chunk, row)
TF_DEVICE void tf_locate(const TfLayout& L, int g, int& p, int& i) {
    int big = L.rem * (L.mbase + 1);
    if (g < big) { p = g / (L.mbase + 1); i = g - p * (L.mbase + 1); }
    else { int h = g - big; p = L.rem + h / L.mbase; i = h - (h / L.mbase) * L.mbase; }
}
