// Device probes: per-step reductions of model expressions over the nodes of every system.
//
// A probe is an expression in the model's string language, lowered by codegen.lower_probes to
// the per-node body tf_eval_probe (same emitter as tf_eval_F: the per-node values are the bits
// the reference's lambdified NumPy code computes), and a reduction over the nodes of a system.
// The generated probe block defines TF_NPROBE, TF_NPROBE_HC, TF_PROBE_USES_X, tf_probe_kind[]
// and tf_eval_probe before this header is read; a model code object without probes compiles
// the no-op defaults below (every code object holds every kernel of the table, tf_args.h).
//
// This file holds what the host harness of the test suite (tests/probe_host/) also compiles
// with g++: the reduction algebra and the walk of one thread along its chunk, on the node window
// that the probes share with the recorders (tf_node.h).  The shuffle / LDS trees and the ring
// hand-over are in tf_entry_hip.h (tfk_probe_partial, tfk_probe_final).
#pragma once
#include "tf_node.h"

#ifndef TF_NPROBE
#define TF_NPROBE 0
#define TF_NPROBE_HC 0
#define TF_PROBE_USES_X 0
static constexpr int tf_probe_kind[1] = {0};
TF_DEVICE void tf_eval_probe(const double (&)[TF_NVAR + TF_NH][2 * TF_MP + 1], const double*,
                             const double*, double, double, double*) {}
#endif
#define TF_NPROBE_A (TF_NPROBE > 0 ? TF_NPROBE : 1)

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
// numpy's answer; the sums are added in a fixed order (the trees of tf_entry_hip.h).
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
TF_DEVICE void tf_probe_walk(const TfProbeArgs& a, int e, int p, int sg, TfProbeAcc (&acc)[TF_NPROBE_A],
                             double* nodes = nullptr) {
    const TfLayout& L = a.L;
    const int len = tf_len(L, p);
    const int gstart = tf_start(L, p);
    const int i0 = sg * TF_PROBE_SEG;
    TfNodeWindow<TF_NPROBE_HC, TF_PROBE_USES_X> W(a, e);
#pragma unroll
    for (int k = 0; k < TF_NPROBE_A; ++k) acc[k] = tf_probe_identity(tf_probe_kind[k]);
    if (i0 >= len) return;
    W.prime(p, len, i0);
#pragma unroll
    for (int j = 0; j < TF_PROBE_SEG; ++j) {
        const int i = i0 + j;
        if (i >= len) break;
        W.advance(p, len, i);
        double v[TF_NPROBE_A];
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
