// TEST-ONLY host harness of the device extrema: the generated extrema block (codegen.lower_extrema) and
// csrc/tf_extrema.h compiled with g++ -- the per-node bodies, the rule and the walk of one thread run as they
// do on the GPU, one call per thread of the kernels' grid.  The integer arithmetic between the two walks is
// the kernels': per workgroup of 256 threads the sum of the counts (tfk_extrema_count); then
// (tfk_extrema_write) a workgroup's base is the sum of the sums of the workgroups before it in its own
// system, the counts of a wavefront go through the 64-lane inclusive scan in its steps (off = 1, 2, ... 32;
// a lane adds the value `off` lanes below), the exclusive offset is that minus the lane's own count, and the
// totals of the wavefronts before it are added.  A thread walks again only when it has entries below
// max_count.  What this checks is the rule, the walk and the arithmetic of the offsets: the loops below are a
// copy of the scan, not the kernels' own tf_ext_wave_sum / tf_ext_wave_scan, which are shuffles and exist
// only under hipcc.  The kernels' scan itself is checked by tests/test_gpu_extrema.py alone (its rough states
// of 20 011 nodes with max_count = 8192 and the run at 100 003 nodes cross several workgroups).  Built per set by tests/extrema_host/build_extrema_host.py; never part of libtriflow_hip.so.
#include "observer_host.h"
#include "tf_extrema.h"

namespace {
void wave_scan(int* v) {
    for (int off = 1; off < 64; off <<= 1) {
        int n[64];
        for (int l = 0; l < 64; ++l) n[l] = l >= off ? v[l] + v[l - off] : v[l];
        for (int l = 0; l < 64; ++l) v[l] = n[l];
    }
}
}  // namespace

extern "C" {

int extrema_host_next() { return TF_NEXT; }
int extrema_host_max_count() { return TF_EXT_MAX_COUNT; }

// the rule alone
int extrema_host_is(int kind, double threshold, double vl, double vc, double vr) {
    return tf_ext_is(kind, threshold, vl, vc, vr) ? 1 : 0;
}

// out[nsys][1 + 4 * max_count]: one row of expression `which` (the entries past the count are left as they
// were); walks[1]: the threads that walked a second time
int extrema_host_run(const TfLayout* Lp, const double* fields, const double* helpers, const double* parvec,
                     const double* parsca, const double* dx, const double* xcoord, const double* hc,
                     int which, int kind, double threshold, int max_count, double* out, int* walks) {
    const TfLayout& L = *Lp;
    if (max_count < 1 || max_count > TF_EXT_MAX_COUNT || L.N < 3) return 1;
    const int nblk = (L.P + 255) / 256;
    std::vector<int> counts((size_t)L.nsys * nblk * 256, -1), sums((size_t)L.nsys * nblk, -1);
    TfExtremaArgs a{};
    static_cast<TfNodeArgs&>(a) = host_node_args(Lp, fields, helpers, parvec, parsca, dx, xcoord, hc);
    a.which = which; a.kind = kind; a.max_count = max_count; a.nblk = nblk; a.row = 0; a.capacity = 1;
    a.threshold = threshold; a.counts = counts.data(); a.sums = sums.data(); a.ring = out;
    for (int e = 0; e < L.nsys; ++e)                                       // tfk_extrema_count
        for (int blk = 0; blk < nblk; ++blk) {
            int part[4] = {0, 0, 0, 0};
            for (int t = 0; t < 256; ++t) {
                const int p = blk * 256 + t;
                const int c = p < L.P ? tf_extrema_count(a, e, p) : 0;
                counts[((size_t)e * nblk + blk) * 256 + t] = c;
                part[t >> 6] += c;
            }
            sums[(size_t)e * nblk + blk] = (part[0] + part[1]) + (part[2] + part[3]);
        }
    *walks = 0;
    for (int e = 0; e < L.nsys; ++e)                                       // tfk_extrema_write
        for (int blk = 0; blk < nblk; ++blk) {
            int before = 0, all = 0;
            for (int b = 0; b < nblk; ++b) {
                all += sums[(size_t)e * nblk + b];
                if (b < blk) before += sums[(size_t)e * nblk + b];
            }
            const int* c = &counts[((size_t)e * nblk + blk) * 256];
            int incl[256], part[4];
            for (int t = 0; t < 256; ++t) incl[t] = c[t];
            for (int w = 0; w < 4; ++w) { wave_scan(incl + 64 * w); part[w] = incl[64 * w + 63]; }
            if (blk == 0) tf_extrema_row(a, e)[0] = (double)all;
            for (int t = 0; t < 256; ++t) {
                const int p = blk * 256 + t;
                int offset = before + (incl[t] - c[t]);
                for (int w = 0; w < (t >> 6); ++w) offset += part[w];
                if (p < L.P && c[t] > 0 && offset < max_count) { tf_extrema_store(a, e, p, offset); ++*walks; }
            }
        }
    return 0;
}

}  // extern "C"
