// Device probes: per-step reductions of model expressions over the nodes of every system.
//
// A probe is an expression in the model's string language, lowered by codegen.lower_probes to
// the per-node body tf_eval_probe (same emitter as tf_eval_F: the per-node values are the bits
// the reference's lambdified NumPy code computes), and a reduction over the nodes of a system.
// The generated probe block defines TF_NPROBE, TF_NPROBE_HC, TF_PROBE_USES_X, tf_probe_kind[]
// and tf_eval_probe before this header is read: it is the tail of a probe code object's
// translation unit and of no other.
//
// The reduction algebra and the walk of one thread along its chunk, on the node window that the
// probes share with the other observers (tf_node.h), are what the host harness of the test suite
// (tests/probe_host/) also compiles with g++; the kernels, with the shuffle / LDS trees and the store
// into the ring, are at the end of the file.
#pragma once
#include "tf_node.h"

#define TF_NPROBE_A TF_NPROBE      // extent of a thread's accumulators (the host harness names it)

// Running state of one reduction: the value and, for argmax / argmin, the natural node index it was
// met at.  Sums ignore the index.
typedef TfNodeAcc TfProbeAcc;

TF_DEVICE bool tf_probe_summed(int kind) { return kind <= TF_PROBE_INTEGRAL; }

TF_DEVICE TfProbeAcc tf_probe_identity(int kind) {
    const double inf = __builtin_inf();
    if (tf_probe_summed(kind)) return {0.0, 0.0};
    const bool up = kind == TF_PROBE_MAX || kind == TF_PROBE_ARGMAX;
    return {up ? -inf : inf, inf};
}

// b after a: the reduction of the two.  Maxima / minima follow numpy: NaN wins (max, min: tf_node_extremum),
// the first NaN wins (argmax, argmin), among equal values the smallest node index wins.  For every
// kind but the sums the result does not depend on the order of the operands, so any tree gives
// numpy's answer; the sums are added in a fixed order (the trees of the kernels below).
TF_DEVICE TfProbeAcc tf_probe_combine(int kind, TfProbeAcc a, TfProbeAcc b) {
    if (tf_probe_summed(kind)) return {a.v + b.v, 0.0};
    const bool anan = a.v != a.v, bnan = b.v != b.v;
    if (kind == TF_PROBE_MAX || kind == TF_PROBE_MIN) return tf_node_extremum(kind == TF_PROBE_MAX, a, b);
    bool take;
    if (anan) take = bnan && b.i < a.i;
    else if (bnan) take = true;
    else take = (kind == TF_PROBE_ARGMAX ? b.v > a.v : b.v < a.v) || (b.v == a.v && b.i < a.i);
    return take ? b : a;
}

// What a reduction becomes once every node is in: mean = sum / N, integral = dx * (sum - (f_0 +
// f_{N-1}) / 2) (np.trapz with a uniform spacing; periodic grids: dx * sum), argmax / argmin =
// x of the node (xnode: its coordinate, looked up by the caller).
TF_DEVICE double tf_probe_finish(int kind, TfProbeAcc r, int N, int periodic, double dx,
                                 double f0, double fN1, double xnode) {
    switch (kind) {
    case TF_PROBE_MEAN: return r.v / (double)N;
    case TF_PROBE_INTEGRAL: return periodic ? dx * r.v : dx * (r.v - (f0 + fN1) / 2.0);
    case TF_PROBE_ARGMAX:
    case TF_PROBE_ARGMIN: return xnode;
    default: return r.v;
    }
}

// One thread, segment sg (TF_PROBE_SEG nodes) of chunk p of system e: the node window (tf_node.h) slides
// along the segment, every node's probe values are folded into acc in node order.  The chunks that own
// natural nodes 0 and N-1 also leave f there in a.ends (the integral's end correction).  NODES (the host
// harness of the tests only): every node's values also go to nodes[(k * nsys + e) * N + natural index].
template <bool NODES = false>
TF_DEVICE void tf_probe_walk(const TfProbeArgs& a, int e, int p, int sg, TfProbeAcc (&acc)[TF_NPROBE],
                             double* nodes = nullptr) {
    const TfLayout& L = a.L;
    const int len = tf_len(L, p);
    const int gstart = tf_start(L, p);
    const int i0 = sg * TF_PROBE_SEG;
    TfNodeWindow<TF_NPROBE_HC, TF_PROBE_USES_X> W(a, e);
#pragma unroll
    for (int k = 0; k < TF_NPROBE; ++k) acc[k] = tf_probe_identity(tf_probe_kind[k]);
    if (i0 >= len) return;
    W.prime(p, len, i0);
#pragma unroll
    for (int j = 0; j < TF_PROBE_SEG; ++j) {
        const int i = i0 + j;
        if (i >= len) break;
        W.advance(p, len, i);
        double v[TF_NPROBE];
        tf_eval_probe(W.w, W.par, W.hc, W.dx, W.xc, v);
        const double gi = (double)(gstart + i);
#pragma unroll
        for (int k = 0; k < TF_NPROBE; ++k) {
            if (NODES) nodes[((int64_t)k * L.nsys + e) * L.N + gstart + i] = v[k];
            acc[k] = tf_probe_combine(tf_probe_kind[k], acc[k], TfProbeAcc{v[k], gi});
            if (tf_probe_kind[k] == TF_PROBE_INTEGRAL) {
                double* end = a.ends + ((int64_t)e * TF_NPROBE + k) * 2;
                if (gstart + i == 0) end[0] = v[k];
                if (gstart + i == L.N - 1) end[1] = v[k];
            }
        }
    }
}

#if defined(__HIPCC__)
// tfk_probe_partial: grid (nsys * nblk, nseg), 256 threads, one thread per segment of a level-1 chunk.
// The chunk walks of a workgroup reduce through a 64-lane shuffle tree (every lane ends with the same
// value: the partner sums are the same two operands) and LDS across the four wavefronts, in a fixed
// order; one (value, index) pair per workgroup, probe and system leaves with plain stores.  No atomics on
// floating-point data: the series are bitwise reproducible.
TF_DEVICE TfProbeAcc tf_probe_wave(int kind, TfProbeAcc r) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const TfProbeAcc o{__shfl_xor(r.v, off, 64), __shfl_xor(r.i, off, 64)};
        r = tf_probe_combine(kind, r, o);
    }
    return r;
}
extern "C" __global__ void __launch_bounds__(256) tfk_probe_partial(TfProbeArgs a) {
    const int e = blockIdx.x / a.nblk, blk = blockIdx.x - e * a.nblk, sg = blockIdx.y;
    const int p = blk * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    TfProbeAcc acc[TF_NPROBE];
    if (p < a.L.P) tf_probe_walk(a, e, p, sg, acc);
    else {
#pragma unroll
        for (int k = 0; k < TF_NPROBE; ++k) acc[k] = tf_probe_identity(tf_probe_kind[k]);
    }
    __shared__ double lv[4][TF_NPROBE], li[4][TF_NPROBE];
#pragma unroll
    for (int k = 0; k < TF_NPROBE; ++k) {
        const TfProbeAcc r = tf_probe_wave(tf_probe_kind[k], acc[k]);
        if (lane == 0) { lv[wave][k] = r.v; li[wave][k] = r.i; }
    }
    __syncthreads();
    if (threadIdx.x < TF_NPROBE) {
        const int k = threadIdx.x, kind = tf_probe_kind[k];
        TfProbeAcc r{lv[0][k], li[0][k]};
        for (int w = 1; w < 4; ++w) r = tf_probe_combine(kind, r, TfProbeAcc{lv[w][k], li[w][k]});
        double* out = a.partial + (((int64_t)e * TF_NPROBE + k) * a.nseg * a.nblk + sg * a.nblk + blk) * 2;
        out[0] = r.v;
        out[1] = r.i;
    }
}
// grid (nsys), 256 threads: wavefront w reduces probes w, w + 4, ... of one system -- the
// partials in a fixed order, strided over the lanes, then the shuffle tree -- and lane 0 writes the finished
// value into row a.row of the ring.  The row comes by value, from the host's count of the rows: the
// launch is queued on the solver's stream between the steps, never inside a captured graph (a replay
// would write every row where it was captured).
extern "C" __global__ void __launch_bounds__(256) tfk_probe_final(TfProbeArgs a) {
    const int e = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const TfLayout& L = a.L;
    const int nb = a.nblk * a.nseg;
    for (int k = wave; k < TF_NPROBE; k += 4) {
        const int kind = tf_probe_kind[k];
        const double* part = a.partial + ((int64_t)e * TF_NPROBE + k) * nb * 2;
        TfProbeAcc r = tf_probe_identity(kind);
        // (eight partials per lane loaded before they are combined, in the same order: one at a time, the
        // loop was a chain of HBM round trips, 6.9 us at config 3)
        for (int b0 = lane; b0 < nb; b0 += 64 * 8) {
            TfProbeAcc v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int b = b0 + 64 * j;
                v[j] = b < nb ? TfProbeAcc{part[2 * b], part[2 * b + 1]} : tf_probe_identity(kind);
            }
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (b0 + 64 * j < nb) r = tf_probe_combine(kind, r, v[j]);
        }
        r = tf_probe_wave(kind, r);
        if (lane == 0) {
            double xnode = 0.0;
            if ((kind == TF_PROBE_ARGMAX || kind == TF_PROBE_ARGMIN) && r.i >= 0.0 && r.i < (double)L.N) {
                int p, i;
                tf_locate(L, (int)r.i, p, i);
                xnode = a.xcoord[tf_idx(L, e * L.P + p, i)];
            }
            const double* end = a.ends + ((int64_t)e * TF_NPROBE + k) * 2;
            const double f0 = kind == TF_PROBE_INTEGRAL ? end[0] : 0.0;
            const double fN1 = kind == TF_PROBE_INTEGRAL ? end[1] : 0.0;
            const double val = tf_probe_finish(kind, r, L.N, L.periodic, a.dx[e], f0, fN1, xnode);
            if (a.row >= 0 && a.row < a.capacity) a.ring[((int64_t)a.row * L.nsys + e) * TF_NPROBE + k] = val;
        }
    }
}
#endif
