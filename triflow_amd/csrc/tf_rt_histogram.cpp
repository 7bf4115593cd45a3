// Host runtime of libtriflow_hip: device histograms (tf_histogram_*).  A histogram set is one more code
// object of the solver's model -- the model's generated body, the generated histogram block
// (codegen.lower_histograms) and tf_histogram.h -- that holds tfk_hist_partial / tfk_hist_final, launched on the
// solver's stream, on one of its state slots (tf_observer, tf_solver.h: what the histograms share with the
// other observers): the two launches per histogram that is due, one row [nsys][nbins + 3] of counts per
// record.
//
// The two kernels are not in the kernel table (tf_args.h).  They are
// looked up by name in the set's own code object when the handle is created (tfb::kernel_lookup) and
// launched through what the lookup returned, so they have no launch id, no bit of the timing mask and no
// line in tf_timing_get: a kernel trace times them.
//
// A histogram owns its edges (a device buffer: the code object does not know them), the counts of its
// workgroups and a ring of rows in device memory, counted on the host (RowRing, tf_solver.h).
#include "tf_solver.h"

#include <cmath>

namespace tfb {
// (a back end without the by-name seam -- the emulation of the test suite -- links these)
__attribute__((weak)) Function* kernel_lookup(Module*, const char* name) {
    throw std::runtime_error(std::string("kernels outside the kernel table (") + name +
                             ") are not supported by this back end");
}
__attribute__((weak)) void launch_function(Function*, unsigned, unsigned, unsigned, const void*, size_t, Stream*) {
    throw std::runtime_error("kernels outside the kernel table are not supported by this back end");
}
}  // namespace tfb

namespace {
struct Histogram {
    int expr = 0, nbins = 0, start = 0, stop = 0, step = 1;
    bool have_edges = false;
    DevBuf edges, partial;                     // partial: uint32 [nsys][nseg * nblk][nbins + 3] in a buffer of doubles
    RowRing ring;                              // a row: nsys * (nbins + 3) doubles
};
}  // namespace

struct tf_histogram : tf_observer {
    int nblk = 0, nseg = 0;
    tfb::Function* fn_partial = nullptr;     // tfk_hist_partial, tfk_hist_final of the set's code object
    tfb::Function* fn_final = nullptr;
    std::vector<std::unique_ptr<Histogram>> hists;
};

extern "C" {

int tf_histogram_create(tf_solver* s, const void* code_object, size_t code_size, int32_t nhist,
                        const int32_t* geometry, int32_t nconst, tf_histogram** out) {
    TF_API_BEGIN
    require(s && out && geometry && code_object, "null argument");
    require(nhist >= 1 && nhist <= 64, "tf_histogram_create: 1 ... 64 histograms");
    require(nconst >= 0, "tf_histogram_create: bad constant count");
    std::unique_ptr<tf_histogram> p(new tf_histogram());
    int nexpr = 0;
    const int N = s->L1.N;
    for (int k = 0; k < nhist; ++k) {
        const int32_t* g = geometry + 6 * k;
        p->hists.emplace_back(new Histogram());
        Histogram& h = *p->hists[k];
        h.expr = g[0]; h.nbins = g[1]; h.ring.capacity = g[2]; h.start = g[3]; h.stop = g[4]; h.step = g[5];
        tf_observer::require_numbered_in_order(
            h.expr, nexpr, "tf_histogram_create: expressions are numbered in the order the histograms first use them");
        require(h.nbins >= 1 && h.nbins <= TF_HIST_MAX_BINS, "tf_histogram_create: 1 ... 256 bins per histogram");
        require(h.ring.capacity >= 1, "tf_histogram_create: a ring has one row at least");
        require(h.step >= 1 && h.start >= 0 && h.start <= N && h.stop >= 0 && h.stop <= N,
                "tf_histogram_create: the window is slice.indices(N) with a step >= 1");
    }
    p->init(s, code_object, code_size, nconst, 0, 0);
    p->fn_partial = tfb::kernel_lookup(p->module, "tfk_hist_partial");
    p->fn_final = tfb::kernel_lookup(p->module, "tfk_hist_final");
    p->nblk = (int)tf_solver::cdiv(s->L1.P, 256);
    p->nseg = (int)tf_solver::cdiv(s->L1.M, TF_PROBE_SEG);
    for (auto& hp : p->hists) {
        Histogram& h = *hp;
        h.ring.row = (size_t)s->nsys * (h.nbins + 3);
        h.edges.alloc((size_t)h.nbins + 1, p->bytes);
        h.partial.alloc(((size_t)s->nsys * p->nseg * p->nblk * (h.nbins + 3) + 1) / 2, p->bytes);
        h.ring.alloc(p->bytes);
    }
    *out = p.release();
    TF_API_END
}

void tf_histogram_destroy(tf_histogram* p) { delete p; }

int tf_histogram_set_consts(tf_histogram* p, const double* values, int32_t nconst) {
    TF_API_BEGIN
    require(p && (values || nconst == 0), "null argument");
    p->set_consts("tf_histogram", values, nconst);
    TF_API_END
}

int tf_histogram_set_x(tf_histogram* p, const double* x) {
    TF_API_BEGIN
    require(p && x, "null argument");
    p->set_x(x);
    TF_API_END
}

int tf_histogram_set_edges(tf_histogram* p, int32_t which, const double* edges, int32_t nedges) {
    TF_API_BEGIN
    require(p && edges, "null argument");
    require(which >= 0 && which < (int)p->hists.size(), "tf_histogram_set_edges: no such histogram");
    Histogram& h = *p->hists[which];
    require(nedges == h.nbins + 1, "tf_histogram_set_edges: nbins + 1 edges, nbins as in tf_histogram_create");
    for (int k = 0; k < nedges; ++k) {                 // (the bisection of tf_hist_classify relies on the order)
        require(std::isfinite(edges[k]), "tf_histogram_set_edges: an edge is not finite");
        require(k == 0 || edges[k - 1] < edges[k], "tf_histogram_set_edges: the edges are not strictly increasing");
    }
    tfb::h2d(h.edges.p, edges, (size_t)nedges * sizeof(double), p->solver->stream);
    h.have_edges = true;
    TF_API_END
}

int tf_histogram_record(tf_histogram* p, int32_t which, int32_t slot) {
    TF_API_BEGIN
    require(p, "null histogram");
    require(which >= 0 && which < (int)p->hists.size(), "tf_histogram_record: no such histogram");
    tf_solver* s = p->solver;
    Histogram& h = *p->hists[which];
    require(h.have_edges, "tf_histogram_record: set_edges first");
    const int row = h.ring.next_row(s->stream);
    TfHistArgs a;
    std::memset(&a, 0, sizeof a);
    static_cast<TfNodeArgs&>(a) = p->node_args(slot);
    a.which = h.expr;
    a.nbins = h.nbins;
    a.nblk = p->nblk;
    a.nseg = p->nseg;
    a.row = row;
    a.capacity = h.ring.capacity;
    a.start = h.start; a.stop = h.stop; a.step = h.step;
    a.edges = h.edges.p;
    a.partial = (unsigned*)h.partial.p;
    a.ring = h.ring.ring.p;
    tfb::launch_function(p->fn_partial, (unsigned)(s->nsys * p->nblk), (unsigned)p->nseg, 256, &a, sizeof a, s->stream);
    // (TF_HIST_FINAL_BLOCK of tf_histogram.h: 16 wavefronts over 64 counters each)
    tfb::launch_function(p->fn_final, (unsigned)s->nsys, (unsigned)tf_solver::cdiv(h.nbins + 3, 64), 1024, &a, sizeof a,
                         s->stream);
    ++h.ring.on_device;
    TF_API_END
}

int tf_histogram_fetch(tf_histogram* p, int32_t which, double* out, int64_t max_rows, int64_t* rows) {
    TF_API_BEGIN
    require(p && rows && (out || max_rows == 0), "null argument");
    require(which >= 0 && which < (int)p->hists.size(), "tf_histogram_fetch: no such histogram");
    p->hists[which]->ring.fetch(p->solver->stream, out, max_rows, rows);
    TF_API_END
}

int tf_histogram_pending(tf_histogram* p, int32_t which, int64_t* rows) {
    TF_API_BEGIN
    require(p && rows, "null argument");
    require(which >= 0 && which < (int)p->hists.size(), "tf_histogram_pending: no such histogram");
    *rows = p->hists[which]->ring.pending();
    TF_API_END
}

}  // extern "C"
