// Device statistics: per-node statistics over time of model expressions (the mean film thickness, the
// envelope max_t h(x), the variance at every node, the time each node saw its crest).
//
// A statistic is an expression in the model's string language, lowered by codegen.lower_statistics to one
// case of tf_eval_stat (same emitter as tf_eval_F, tf_eval_probe and tf_eval_record: the per-node values
// are the bits the reference's lambdified NumPy code computes), and a kind (TF_STAT_*, tf_args.h).  The
// generated statistic block defines TF_NSTAT, TF_NSTAT_HC, TF_STAT_USES_X and tf_eval_stat before this
// header is read: it is the tail of a statistic code object's translation unit and of no other.
//
// The fold of one sample and the walk of one thread (on the node window the statistics share with the
// probes and the recorders, tf_node.h) are what the host harness of the test suite (tests/stat_host/)
// also compiles with g++; the kernel itself is at the end of the file.
#pragma once
#include "tf_node.h"

// Sample k (1, 2, ... as a double) with value v at time t into the accumulators of one node: a0 its
// element of plane 0, a1 of plane 1 (kinds of two planes only, tf_stat_planes).  Sample 1 is written and
// nothing is read: accumulators start over without being cleared.  The recurrences are the definition
// (DESIGN.md section 17); no operation is contracted (-ffp-contract=off), so NumPy folding the same
// values gives the same bits.
TF_DEVICE void tf_stat_fold(int kind, double k, double t, double v, double* a0, double* a1) {
    const bool first = k == 1.0;
    switch (kind) {
    case TF_STAT_MEAN: {
        const double m = first ? v : *a0;
        *a0 = first ? v : m + (v - m) / k;
    } break;
    case TF_STAT_VAR: {
        if (first) { *a0 = v; *a1 = 0.0; break; }
        const double m = *a0, d = v - m;
        const double mk = m + d / k;
        *a0 = mk;
        *a1 = *a1 + d * (v - mk);
    } break;
    case TF_STAT_MAX:
    case TF_STAT_MIN:
        *a0 = first ? v : tf_node_extremum(kind == TF_STAT_MAX, TfNodeAcc{*a0, 0.0}, TfNodeAcc{v, 0.0}).v;
        break;
    default: {                                 // argmax, argmin: the first sample at the extremum, the first NaN
        if (first) { *a0 = v; *a1 = t; break; }
        const double c = *a0;
        const bool take = c == c && (v != v || (kind == TF_STAT_ARGMAX ? v > c : v < c));
        if (take) { *a0 = v; *a1 = t; }
    } break;
    }
}

// One thread, segment sg (TF_PROBE_SEG nodes) of chunk p of system e: the node window (tf_node.h) slides
// along the segment, every node's value is folded into the node's own elements of the accumulator planes.
TF_DEVICE void tf_stat_walk(const TfStatArgs& a, int e, int p, int sg) {
    const TfLayout& L = a.L;
    const int len = tf_len(L, p);
    const int i0 = sg * TF_PROBE_SEG;
    if (i0 >= len) return;
    TfNodeWindow<TF_NSTAT_HC, TF_STAT_USES_X> W(a, e);
    W.prime(p, len, i0);
#pragma unroll
    for (int j = 0; j < TF_PROBE_SEG; ++j) {
        const int i = i0 + j;
        if (i >= len) break;
        W.advance(p, len, i);
        const double v = tf_eval_stat(a.which, W.w, W.par, W.hc, W.dx, W.xc);
        const int64_t s = tf_idx(L, e * L.P + p, i);
        tf_stat_fold(a.kind, a.k, a.t, v, a.acc + s, a.acc + L.plane + s);
    }
}

#if defined(__HIPCC__)
// grid (nsys * nblk, nseg), 256 threads, one launch per statistic that is due: thread x of workgroup blk
// walks segment blockIdx.y of chunk blk * 256 + x, as in tfk_probe_partial -- the lanes of a wavefront
// sit over neighbouring chunks, so every load of the state and every load and store of the accumulators
// is 512 contiguous bytes.  An element of the planes belongs to one node and a node to one thread: no
// atomics, no LDS, no cursor, and the planes are bitwise reproducible.  k and t come by value, from the
// host's count of the samples: the launch is queued on the solver's stream between the steps, never
// inside a captured graph (a replay would fold every sample as the one it was captured with).
extern "C" __global__ void __launch_bounds__(256) tfk_stat(TfStatArgs a) {
    const int e = blockIdx.x / a.nblk, blk = blockIdx.x - e * a.nblk;
    const int p = blk * 256 + threadIdx.x;
    if (p < a.L.P) tf_stat_walk(a, e, p, (int)blockIdx.y);
}
#endif
