// Device recorders: decimated space-time series of model expressions (h(x, t) of a film, a kymograph).
//
// A recorder is an expression in the model's string language, lowered by codegen.lower_records to one
// case of tf_eval_record (same emitter as tf_eval_F and tf_eval_probe: the per-node values are the bits
// the reference's lambdified NumPy code computes), a window of nodes start:stop:step and a pool over the
// nodes of each bin (TF_REC_*, tf_args.h).  The generated record block defines TF_NREC, TF_NREC_HC,
// TF_REC_USES_X and tf_eval_record before this header is read: it is the tail of a record code object's
// translation unit and of no other.
//
// The walk (on the node window the recorders share with the probes, tf_node.h) and the combine are what the host harness of the test suite (tests/record_host/) also
// compiles with g++; the kernel itself is at the end of the file.
#pragma once
#include "tf_node.h"

// b after a.  Maxima / minima as numpy has them (tf_node_extremum: NaN wins; the order of the operands
// does not matter), the mean's sum is added in the order the caller fixes.
TF_DEVICE double tf_rec_combine(int pool, double a, double b) {
    if (pool == TF_REC_MEAN) return a + b;
    return tf_node_extremum(pool == TF_REC_MAX, TfNodeAcc{a, 0.0}, TfNodeAcc{b, 0.0}).v;
}

// nodes of bin j ("sample": its first node only)
TF_DEVICE int tf_rec_count(const TfRecordArgs& a, int j) {
    if (a.pool == TF_REC_SAMPLE) return 1;
    const int g0 = a.start + j * a.step;
    return (a.stop - g0 < a.step ? a.stop : g0 + a.step) - g0;
}

// One thread: the natural nodes g0 ... g0 + n - 1 (n >= 1, inside the system) of system e, folded in node
// order.  The node window (tf_node.h) slides along them; a walk that leaves its chunk goes on at row 0 of
// the next one with the window it holds.
TF_DEVICE double tf_record_walk(const TfRecordArgs& a, int e, int g0, int n) {
    const TfLayout& L = a.L;
    int p, i;
    tf_locate(L, g0, p, i);
    int len = tf_len(L, p);
    TfNodeWindow<TF_NREC_HC, TF_REC_USES_X> W(a, e);
    W.prime(p, len, i);
    double acc = 0.0;
    for (int j = 0; j < n; ++j) {
        W.advance(p, len, i);
        const double v = tf_eval_record(a.which, W.w, W.par, W.hc, W.dx, W.xc);
        acc = j == 0 ? v : tf_rec_combine(a.pool, acc, v);
        if (++i == len && p + 1 < L.P) { ++p; i = 0; len = tf_len(L, p); }
    }
    return acc;
}

// part s of bin j: nodes s * part ... of the bin (the caller checks that the part holds a node)
TF_DEVICE double tf_record_part(const TfRecordArgs& a, int e, int j, int s) {
    const int cnt = tf_rec_count(a, j), lo = s * a.part;
    return tf_record_walk(a, e, a.start + j * a.step + lo, cnt - lo < a.part ? cnt - lo : a.part);
}

// the parts of bin j, in their order, to the value of column j
TF_DEVICE double tf_record_finish(const TfRecordArgs& a, int j, const double* parts) {
    const int cnt = tf_rec_count(a, j);
    double acc = parts[0];
    for (int s = 1; s * a.part < cnt; ++s) acc = tf_rec_combine(a.pool, acc, parts[s]);
    return a.pool == TF_REC_MEAN ? acc / (double)cnt : acc;
}

#if defined(__HIPCC__)
// grid (nsys * nblk), TF_REC_BLOCK threads: `split` neighbouring threads share a bin, thread s of them
// walks `part` nodes of it (at most 8 where the bin allows: the threads of a wavefront then read a few
// whole rows of neighbouring chunks, and a bin of 64 nodes keeps 8 threads busy instead of one); the
// parts meet in LDS and the first TF_REC_BLOCK / split threads combine them in part order and store the
// columns of the workgroup side by side in row a.row of the ring.  The row comes by value, as the probes'
// does, from the host's count of the rows, which wraps at the ring's capacity: the launch is queued on the
// solver's stream between the steps, never inside a captured graph.  No atomics.
extern "C" __global__ void __launch_bounds__(TF_REC_BLOCK) tfk_record(TfRecordArgs a) {
    __shared__ double parts[TF_REC_BLOCK];
    const int e = blockIdx.x / a.nblk, blk = blockIdx.x - e * a.nblk;
    const int cpb = TF_REC_BLOCK / a.split;
    const int c = threadIdx.x / a.split, s = threadIdx.x - c * a.split;
    const int j = blk * cpb + c;
    double v = 0.0;
    if (j < a.ncols && s * a.part < tf_rec_count(a, j)) v = tf_record_part(a, e, j, s);
    parts[threadIdx.x] = v;
    __syncthreads();
    const int jj = blk * cpb + threadIdx.x;
    if (threadIdx.x < cpb && jj < a.ncols && a.row >= 0 && a.row < a.capacity)
        a.ring[((int64_t)a.row * a.L.nsys + e) * a.ncols + jj] = tf_record_finish(a, jj, parts + threadIdx.x * a.split);
}
#endif
