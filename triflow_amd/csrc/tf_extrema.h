// Device extrema: the crests (or troughs) of a model expression -- where they are, how tall, how many -- one
// row of variable length per record, its entries in node order.
//
// The expression is in the model's string language, lowered by codegen.lower_extrema to one case of
// tf_eval_extrema (same emitter as tf_eval_F and the other observers' bodies: the per-node values are the
// bits the reference's lambdified NumPy code computes).  Node g is an extremum of kind max iff
// v[g-1] < v[g] and v[g] > v[g+1], both strictly (min: both reversed), v[g] is finite and beyond the
// threshold; the neighbours wrap on a periodic grid, the end nodes of any other grid are never extrema
// (scipy.signal.argrelextrema with np.greater / np.less, mode "wrap" / "clip").  A NaN compares false, so a
// NaN neighbour disqualifies a node; a plateau of equal values is not reported.  The generated block defines
// TF_NEXT, TF_NEXT_HC, TF_EXT_USES_X and tf_eval_extrema before this header is read: it is the tail of an
// extrema code object's translation unit and of no other.
//
// In the partition-interleaved layout node order is not thread order, so a row is an ordered stream
// compaction in two passes: tfk_extrema_count counts the extrema of every chunk, tfk_extrema_write scans the
// counts (integers only) and repeats the walk, every thread storing its entries at its place in the row.
// The device stores only values it evaluated -- (g, v[g-1], v[g], v[g+1]) -- and the host refines them.
//
// The rule, the walk of one thread (on the node window the extrema share with the other observers,
// tf_node.h) and the stores are what the host harness of the test suite (tests/extrema_host/) also compiles
// with g++ (it copies the scan: the shuffles below exist only under hipcc); the kernels are at the end of
// the file.
#pragma once
#include "tf_node.h"

// Is the node with the value vc between vl and vr an extremum?  Finite: vc - vc is 0.0 for a finite value and
// NaN for an infinity or a NaN.  A NaN among vl, vr fails its comparison.
TF_DEVICE bool tf_ext_is(int kind, double threshold, double vl, double vc, double vr) {
    const bool finite = vc - vc == 0.0;
    if (kind == TF_EXT_MAX) return finite && vl < vc && vc > vr && vc > threshold;
    return finite && vl > vc && vc < vr && vc < threshold;
}

// One thread, chunk p of system e: the walk goes from the last node of the previous chunk to the first node
// of the next one (around the ends of a periodic system; a system that is not periodic has no node there,
// and the NaN that stands in for it keeps nodes 0 and N - 1 from being extrema), the node window continuing
// across the chunk borders as in tf_record_walk.  (vl, vc, vr) slide, so the expression is evaluated once at
// every node of the walk.  emit(g, vl, vc, vr) is called for every extremum of the chunk, in node order;
// returns their number.
template <class Emit>
TF_DEVICE int tf_extrema_walk(const TfExtremaArgs& a, int e, int p, Emit emit) {
    const TfLayout& L = a.L;
    const int len = tf_len(L, p), start = tf_start(L, p);
    const bool has_prev = p > 0 || L.periodic, has_next = p < L.P - 1 || L.periodic;
    const double nan = __builtin_nan("");
    TfNodeWindow<TF_NEXT_HC, TF_EXT_USES_X> W(a, e);
    double vl = nan, vc, vr;
    if (has_prev) {
        const int pp = p > 0 ? p - 1 : L.P - 1, plen = tf_len(L, pp);
        W.prime(pp, plen, plen - 1);
        W.advance(pp, plen, plen - 1);
        vl = tf_eval_extrema(a.which, W.w, W.par, W.hc, W.dx, W.xc);
    } else {
        W.prime(p, len, 0);
    }
    W.advance(p, len, 0);
    vc = tf_eval_extrema(a.which, W.w, W.par, W.hc, W.dx, W.xc);
    int n = 0;
    for (int i = 0; i < len; ++i) {
        vr = nan;
        if (i + 1 < len) {
            W.advance(p, len, i + 1);
            vr = tf_eval_extrema(a.which, W.w, W.par, W.hc, W.dx, W.xc);
        } else if (has_next) {
            const int pn = p < L.P - 1 ? p + 1 : 0;
            W.advance(pn, tf_len(L, pn), 0);
            vr = tf_eval_extrema(a.which, W.w, W.par, W.hc, W.dx, W.xc);
        }
        if (tf_ext_is(a.kind, a.threshold, vl, vc, vr)) {
            emit(start + i, vl, vc, vr);
            ++n;
        }
        vl = vc;
        vc = vr;
    }
    return n;
}

// the extrema of chunk p (tfk_extrema_count)
TF_DEVICE int tf_extrema_count(const TfExtremaArgs& a, int e, int p) {
    return tf_extrema_walk(a, e, p, [](int, double, double, double) {});
}

// The row of system e in the ring: [0] the system's count, then max_count entries of four doubles.
TF_DEVICE double* tf_extrema_row(const TfExtremaArgs& a, int e) {
    return a.ring + ((int64_t)a.row * a.L.nsys + e) * (1 + 4 * (int64_t)a.max_count);
}

// The walk again (tfk_extrema_write): the chunk's extrema are entries offset, offset + 1, ... of the
// system's row; those below max_count are stored.
TF_DEVICE void tf_extrema_store(const TfExtremaArgs& a, int e, int p, int offset) {
    double* row = tf_extrema_row(a, e) + 1;
    const int max_count = a.max_count;
    int at = offset;
    tf_extrema_walk(a, e, p, [&](int g, double vl, double vc, double vr) {
        if (at >= 0 && at < max_count) {
            double* out = row + 4 * (int64_t)at;
            out[0] = (double)g;
            out[1] = vl;
            out[2] = vc;
            out[3] = vr;
        }
        ++at;
    });
}

#if defined(__HIPCC__)
// the sum of an integer over the 64 lanes (every lane ends with it) and the inclusive scan over them
TF_DEVICE int tf_ext_wave_sum(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
TF_DEVICE int tf_ext_wave_scan(int v, int lane) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int t = __shfl_up(v, off, 64);
        if (lane >= off) v += t;
    }
    return v;
}

// grid (nsys * nblk), 256 threads, thread x of workgroup blk walks chunk blk * 256 + x: the lanes of a
// wavefront sit over neighbouring chunks, so every load of the state is 512 contiguous bytes.  The count of
// every chunk (0 for the threads past the last chunk) and the sum of the workgroup leave with plain stores.
extern "C" __global__ void __launch_bounds__(256) tfk_extrema_count(TfExtremaArgs a) {
    __shared__ int part[4];
    const int e = blockIdx.x / a.nblk, blk = blockIdx.x - e * a.nblk;
    const int p = blk * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = p < a.L.P ? tf_extrema_count(a, e, p) : 0;
    a.counts[((int64_t)e * a.nblk + blk) * 256 + threadIdx.x] = c;
    const int s = tf_ext_wave_sum(c);
    if (lane == 0) part[wave] = s;
    __syncthreads();
    if (threadIdx.x == 0) a.sums[(int64_t)e * a.nblk + blk] = (part[0] + part[1]) + (part[2] + part[3]);
}

// Same grid.  The first wavefront adds the sums of the workgroups of its own system, those before this
// workgroup (its base in the row) and all of them (the system's count); the counts of the workgroup's chunks
// go through an exclusive scan over the 64 lanes and LDS across the four wavefronts.  Integers only, no
// atomics, no dependence on the order the workgroups arrive in: a row is the same bits on every run.  A
// thread whose entries all lie past max_count, or that has none, does not walk again.  The row index comes
// by value, from the host's count of the rows: the launch is queued on the solver's stream between the
// steps, never inside a captured graph (a replay would write every row where it was captured).
extern "C" __global__ void __launch_bounds__(256) tfk_extrema_write(TfExtremaArgs a) {
    __shared__ int part[4];
    __shared__ int head[2];
    const int e = blockIdx.x / a.nblk, blk = blockIdx.x - e * a.nblk;
    const int p = blk * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // (before the barrier below: a is the launch's argument, the same for every thread, so the whole
    // workgroup leaves or none of it does -- a condition that differs between threads must not go here)
    if (a.row < 0 || a.row >= a.capacity) return;
    const int c = a.counts[((int64_t)e * a.nblk + blk) * 256 + threadIdx.x];
    const int incl = tf_ext_wave_scan(c, lane);
    if (lane == 63) part[wave] = incl;
    if (wave == 0) {
        const int* sums = a.sums + (int64_t)e * a.nblk;
        int before = 0, all = 0;
        for (int b = lane; b < a.nblk; b += 64) {
            const int s = sums[b];
            all += s;
            if (b < blk) before += s;
        }
        before = tf_ext_wave_sum(before);
        all = tf_ext_wave_sum(all);
        if (lane == 0) { head[0] = before; head[1] = all; }
    }
    __syncthreads();
    int offset = head[0] + (incl - c);
    for (int w = 0; w < wave; ++w) offset += part[w];
    if (blk == 0 && threadIdx.x == 0) tf_extrema_row(a, e)[0] = (double)head[1];
    if (p < a.L.P && c > 0 && offset < a.max_count) tf_extrema_store(a, e, p, offset);
}
#endif
