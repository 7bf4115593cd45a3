// TEST-ONLY host harness of the device histograms: the generated histogram block (codegen.lower_histograms)
// and csrc/tf_histogram.h compiled with g++ -- the per-node bodies, the classification, the window test and
// the walk of one thread run as they do on the GPU, one call per thread of tfk_hist_partial's grid.  The
// counts take the kernels' way: per workgroup of 256 threads one set of nbins + 3 unsigned counters per
// wavefront of 64, the four sets summed into the workgroup's set; per system (tfk_hist_final) the sets of
// its workgroups summed and stored as doubles.  Built per histogram set by
// tests/hist_host/build_hist_host.py; never part of libtriflow_hip.so.
#include "observer_host.h"
#include "tf_histogram.h"

extern "C" {

int hist_host_nhist() { return TF_NHIST; }
int hist_host_max_bins() { return TF_HIST_MAX_BINS; }

// the counter of one value (tf_hist_classify)
int hist_host_classify(double v, const double* edges, int nbins) { return tf_hist_classify(v, edges, nbins); }

// out[nsys][nbins + 3]: one row of expression `which` for the edges and the window; *sets: the workgroups
// of tfk_hist_partial per system
int hist_host_run(const TfLayout* Lp, const double* fields, const double* helpers, const double* parvec,
                  const double* parsca, const double* dx, const double* xcoord, const double* hc,
                  int which, int nbins, const double* edges, int start, int stop, int step, double* out,
                  int* sets) {
    const TfLayout& L = *Lp;
    const int nblk = (L.P + 255) / 256, nseg = (L.M + TF_PROBE_SEG - 1) / TF_PROBE_SEG, nset = nblk * nseg;
    if (nbins < 1 || nbins > TF_HIST_MAX_BINS) return 1;
    const int w = nbins + 3;
    TfHistArgs a{};
    static_cast<TfNodeArgs&>(a) = host_node_args(Lp, fields, helpers, parvec, parsca, dx, xcoord, hc);
    a.which = which; a.nbins = nbins; a.nblk = nblk; a.nseg = nseg;
    a.start = start; a.stop = stop; a.step = step; a.edges = edges;
    std::vector<double> lds(edges, edges + nbins + 1);                 // the workgroup's copy of the edges
    std::vector<unsigned> partial((size_t)L.nsys * nset * w);
    for (int e = 0; e < L.nsys; ++e) {
        for (int sg = 0; sg < nseg; ++sg)                              // tfk_hist_partial
            for (int blk = 0; blk < nblk; ++blk) {
                std::vector<unsigned> cnt((size_t)4 * w, 0u);
                for (int t = 0; t < 256; ++t) {
                    const int p = blk * 256 + t;
                    unsigned* mine = &cnt[(size_t)(t >> 6) * w];
                    if (p < L.P) tf_hist_walk(a, e, p, sg, lds.data(), nbins, [mine](int c) { ++mine[c]; });
                }
                unsigned* o = &partial[(((size_t)e * nseg + sg) * nblk + blk) * w];
                for (int c = 0; c < w; ++c) o[c] = cnt[c] + cnt[w + c] + cnt[2 * w + c] + cnt[3 * w + c];
            }
        for (int c = 0; c < w; ++c) {                                  // tfk_hist_final
            unsigned long long sum = 0;
            for (int b = 0; b < nset; ++b) sum += partial[((size_t)e * nset + b) * w + c];
            out[(size_t)e * w + c] = (double)sum;
        }
    }
    *sets = nset;
    return 0;
}

}  // extern "C"
