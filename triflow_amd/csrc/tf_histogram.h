// Device histograms: the distribution of the values of a model expression over a window of nodes, one row
// of integer counts per record.
//
// A histogram is an expression in the model's string language, lowered by codegen.lower_histograms to one
// case of tf_eval_hist (same emitter as tf_eval_F and the other observers' bodies: the per-node values are
// the bits the reference's lambdified NumPy code computes), a table of nbins + 1 edges in a device buffer of
// the handle and a window of nodes.  The rule (TfHistArgs, tf_args.h): bin i counts edges[i] <= v <
// edges[i + 1], the last bin also v == edges[nbins]; below, above and NaN are counted apart.  That is
// np.histogram(v, bins=edges)[0] for the values it accepts.
//
// The generated histogram block defines TF_NHIST, TF_NHIST_HC, TF_HIST_USES_X and tf_eval_hist before this
// header is read: it is the tail of a histogram code object's translation unit and of no other.  Unlike the
// other observers' kernels, tfk_hist_partial and tfk_hist_final are not in the kernel table (tf_args.h): the
// runtime finds them by name.
//
// The classification (of one value, and of the values of a segment at once), the window test and the walk
// of one thread (on the node window the histograms share with the other observers, tf_node.h) are what the
// host harness of the test suite (tests/hist_host/) also compiles with g++; the kernels are at the end of
// the file.
#pragma once
#include "tf_node.h"

// Counter of the value v among nbins + 3: 0 ... nbins - 1 the bins, nbins: v < edges[0], nbins + 1:
// v > edges[nbins], nbins + 2: NaN.  Comparisons only (so -0.0 is 0.0 and the infinities go below / above):
// inside, a bisection for the last edge that is <= v, kept below nbins so that v == edges[nbins] lands
// in the last bin.  One code path for uniform and for explicit edges; at most 8 steps.
TF_DEVICE int tf_hist_classify(double v, const double* edges, int nbins) {
    if (v != v) return nbins + 2;
    if (v < edges[0]) return nbins;
    if (v > edges[nbins]) return nbins + 1;
    int lo = 0, hi = nbins;                    // edges[lo] <= v, and hi == nbins or v < edges[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (edges[mid] <= v) lo = mid; else hi = mid;
    }
    return lo;
}

// natural node g is one of start, start + step, ... < stop
TF_DEVICE bool tf_hist_in_window(int g, int start, int stop, int step) {
    return g >= start && g < stop && (g - start) % step == 0;
}

// The same rule for the TF_PROBE_SEG values of a segment at once (c[j] is written where bit j of `take` is
// set).  Every bisection starts from the same interval, so all of them are done after the same number of
// halvings, ceil(log2(nbins)): the loop runs that often for every value, without a test of its own -- an
// interval of one bin halves to itself, since edges[lo] <= v holds -- and a step is TF_PROBE_SEG independent
// reads of the edges instead of one.  One value at a time, a thread of tfk_hist_partial waited for the
// table 8 x 6 times in a row at 64 bins.  What is not inside (a NaN compares false and ends at bin 0) is
// put right afterwards by the three comparisons of tf_hist_classify.
TF_DEVICE void tf_hist_classify_segment(const double (&v)[TF_PROBE_SEG], unsigned take, const double* edges,
                                        int nbins, int (&c)[TF_PROBE_SEG]) {
    int lo[TF_PROBE_SEG], hi[TF_PROBE_SEG];
#pragma unroll
    for (int j = 0; j < TF_PROBE_SEG; ++j) { lo[j] = 0; hi[j] = nbins; }
    for (int len = nbins; len > 1; len = (len + 1) >> 1) {
#pragma unroll
        for (int j = 0; j < TF_PROBE_SEG; ++j) {
            const int mid = (lo[j] + hi[j]) >> 1;          // 0 ... nbins - 1: lo < nbins throughout
            if (edges[mid] <= v[j]) lo[j] = mid; else hi[j] = mid;
        }
    }
    const double first = edges[0], last = edges[nbins];
#pragma unroll
    for (int j = 0; j < TF_PROBE_SEG; ++j) {
        if (!((take >> j) & 1u)) continue;
        c[j] = v[j] != v[j] ? nbins + 2 : (v[j] < first ? nbins : (v[j] > last ? nbins + 1 : lo[j]));
    }
}

// One thread, segment sg (TF_PROBE_SEG nodes) of chunk p of system e, as tf_probe_walk: the node window
// slides along the segment and the expression is evaluated once per window node; then the values are
// classified together (tf_hist_classify_segment against `edges`, the caller's copy of a.edges) and
// count(counter) is called once per window node, in node order.
template <class Count>
TF_DEVICE void tf_hist_walk(const TfHistArgs& a, int e, int p, int sg, const double* edges, int nbins,
                            Count&& count) {
    const TfLayout& L = a.L;
    const int len = tf_len(L, p);
    const int gstart = tf_start(L, p);
    const int i0 = sg * TF_PROBE_SEG;
    if (i0 >= len) return;
    // (no window node in the segment: nothing is loaded)
    const int last = gstart + (i0 + TF_PROBE_SEG < len ? i0 + TF_PROBE_SEG : len) - 1;
    if (last < a.start || gstart + i0 >= a.stop) return;
    TfNodeWindow<TF_NHIST_HC, TF_HIST_USES_X> W(a, e);
    W.prime(p, len, i0);
    double v[TF_PROBE_SEG];
    unsigned take = 0u;
#pragma unroll
    for (int j = 0; j < TF_PROBE_SEG; ++j) {
        const int i = i0 + j;
        v[j] = 0.0;
        if (i >= len) continue;
        W.advance(p, len, i);
        if (!tf_hist_in_window(gstart + i, a.start, a.stop, a.step)) continue;
        v[j] = tf_eval_hist(a.which, W.w, W.par, W.hc, W.dx, W.xc);
        take |= 1u << j;
    }
    int c[TF_PROBE_SEG];
    tf_hist_classify_segment(v, take, edges, nbins, c);
#pragma unroll
    for (int j = 0; j < TF_PROBE_SEG; ++j)
        if ((take >> j) & 1u) count(c[j]);
}

#if defined(__HIPCC__)
// grid (nsys * nblk, nseg), 256 threads, one launch per histogram that is due: thread x of workgroup blk
// walks segment blockIdx.y of chunk blk * 256 + x, as in tfk_probe_partial -- the lanes of a wavefront sit
// over neighbouring chunks, so every load of the state is 512 contiguous bytes.  The workgroup copies the
// edges into LDS once; a node's counter is bumped with an LDS integer add, every wavefront in a set of
// counters of its own; after the barrier the four sets are summed and the workgroup's nbins + 3 counts
// leave with plain coalesced stores.  No global atomics and nothing in floating point: a row does not
// depend on the order of arrival.
extern "C" __global__ void __launch_bounds__(256) tfk_hist_partial(TfHistArgs a) {
    __shared__ double edges[TF_HIST_MAX_BINS + 1];
    __shared__ unsigned cnt[4][TF_HIST_MAX_BINS + 3];
    const int e = blockIdx.x / a.nblk, blk = blockIdx.x - e * a.nblk, sg = blockIdx.y;
    const int p = blk * 256 + threadIdx.x;
    const int wave = threadIdx.x >> 6;
    const int nb = a.nbins < 1 ? 1 : (a.nbins < TF_HIST_MAX_BINS ? a.nbins : TF_HIST_MAX_BINS);
    for (int t = threadIdx.x; t <= nb; t += 256) edges[t] = a.edges[t];
    for (int t = threadIdx.x; t < 4 * (TF_HIST_MAX_BINS + 3); t += 256) (&cnt[0][0])[t] = 0u;
    __syncthreads();
    if (p < a.L.P) {
        unsigned* mine = cnt[wave];
        tf_hist_walk(a, e, p, sg, edges, nb, [mine](int c) { atomicAdd(&mine[c], 1u); });
    }
    __syncthreads();
    unsigned* out = a.partial + (((int64_t)e * a.nseg + sg) * a.nblk + blk) * (nb + 3);
    for (int t = threadIdx.x; t < nb + 3; t += 256) out[t] = cnt[0][t] + cnt[1][t] + cnt[2][t] + cnt[3][t];
}
// grid (nsys, ceil((nbins + 3) / 64)), TF_HIST_FINAL_BLOCK threads = 16 wavefronts: the lanes of a wavefront
// sit over 64 neighbouring counters (256 contiguous bytes per load), wavefront k sums the sets k, k + 16, ...
// of its system with eight loads in flight, the 16 sums meet in LDS and the first wavefront stores the
// totals into row a.row of the ring as doubles.  (One workgroup of 256 threads that walked all nseg * nblk
// sets, 492 at 1e6 nodes, eight at a time was a chain of 62 HBM round trips: 25 us at 64 bins, 43 us at
// 256, measured.)  The row comes by value, from the host's count of the rows: the launch is queued on the
// solver's stream between the steps, never inside a captured graph.
#define TF_HIST_FINAL_BLOCK 1024
extern "C" __global__ void __launch_bounds__(TF_HIST_FINAL_BLOCK) tfk_hist_final(TfHistArgs a) {
    __shared__ unsigned long long sums[TF_HIST_FINAL_BLOCK / 64][64];
    const int e = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nb = a.nbins < 1 ? 1 : (a.nbins < TF_HIST_MAX_BINS ? a.nbins : TF_HIST_MAX_BINS);
    const int w = nb + 3, nset = a.nseg * a.nblk;
    const int t = blockIdx.y * 64 + lane;
    const unsigned* part = a.partial + (int64_t)e * nset * w;
    unsigned long long sum = 0;
    if (t < w) {
        for (int b0 = wave; b0 < nset; b0 += 8 * (TF_HIST_FINAL_BLOCK / 64)) {
            unsigned v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int b = b0 + j * (TF_HIST_FINAL_BLOCK / 64);
                v[j] = b < nset ? part[(int64_t)b * w + t] : 0u;
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) sum += v[j];
        }
    }
    sums[wave][lane] = sum;
    __syncthreads();
    if (wave == 0 && t < w) {
        unsigned long long total = 0;
#pragma unroll
        for (int k = 0; k < TF_HIST_FINAL_BLOCK / 64; ++k) total += sums[k][lane];
        if (a.row >= 0 && a.row < a.capacity)
            a.ring[((int64_t)a.row * a.L.nsys + e) * w + t] = (double)total;
    }
}
#endif
