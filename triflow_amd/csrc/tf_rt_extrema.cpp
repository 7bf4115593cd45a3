// Host runtime of libtriflow_hip: device extrema (tf_extrema_*).  An extrema set is one more code object of
// the solver's model -- the model's generated body, the generated extrema block (codegen.lower_extrema)
// and tf_extrema.h -- that holds tfk_extrema_count / tfk_extrema_write, launched on the
// solver's stream, on one of its state slots (tf_observer, tf_solver.h: what the extrema share with the
// other observers): the two launches per observer that is due, one row [nsys][1 + 4 * max_count] per record.
//
// An observer owns the counts of its chunks and workgroups (integers) and a ring of rows in device
// memory, counted on the host (RowRing, tf_solver.h).
#include "tf_solver.h"

namespace {
// rows of a ring the caller gave no capacity for: 1024, or what 32 MB hold
const size_t kDefaultRows = 1024, kDefaultBytes = (size_t)32 << 20;

struct Extrema {
    int expr = 0, kind = 0, max_count = 0;
    double threshold = 0.0;
    DevBuf counts, sums;                       // int32 in buffers of doubles
    RowRing ring;                              // a row: nsys * (1 + 4 * max_count) doubles
};
}  // namespace

struct tf_extrema : tf_observer {
    int nblk = 0;
    std::vector<std::unique_ptr<Extrema>> obs;
};

extern "C" {

int tf_extrema_create(tf_solver* s, const void* code_object, size_t code_size, int32_t next,
                      const int32_t* geometry, const double* thresholds, int32_t nconst, tf_extrema** out) {
    TF_API_BEGIN
    require(s && out && geometry && thresholds && code_object, "null argument");
    require(next >= 1 && next <= 64, "tf_extrema_create: 1 ... 64 observers");
    require(nconst >= 0, "tf_extrema_create: bad constant count");
    require(s->L1.N >= 3, "tf_extrema_create: an extremum has two neighbours, a system three nodes at least");
    std::unique_ptr<tf_extrema> p(new tf_extrema());
    int nexpr = 0;
    for (int k = 0; k < next; ++k) {
        const int32_t* g = geometry + 4 * k;
        p->obs.emplace_back(new Extrema());
        Extrema& ex = *p->obs[k];
        ex.expr = g[0]; ex.kind = g[1]; ex.max_count = g[2]; ex.ring.capacity = g[3];
        ex.threshold = thresholds[k];
        tf_observer::require_numbered_in_order(
            ex.expr, nexpr, "tf_extrema_create: expressions are numbered in the order the observers first use them");
        require(ex.kind == TF_EXT_MAX || ex.kind == TF_EXT_MIN, "tf_extrema_create: kind is max (0) or min (1)");
        require(ex.max_count >= 1 && ex.max_count <= TF_EXT_MAX_COUNT, "tf_extrema_create: max_count is 1 ... 8192");
        require(ex.ring.capacity >= 0, "tf_extrema_create: a ring has one row at least (0: the default)");
        require(ex.threshold == ex.threshold, "tf_extrema_create: the threshold is a NaN");
        ex.ring.row = (size_t)s->nsys * (1 + 4 * (size_t)ex.max_count);
        if (ex.ring.capacity == 0) {
            const size_t fit = kDefaultBytes / (ex.ring.row * sizeof(double));
            require(fit >= 1, "tf_extrema_create: one row of the ring (8 * nsys * (1 + 4 * max_count) bytes) is "
                              "more than the 32 MB of a default ring: a smaller max_count, or a capacity");
            ex.ring.capacity = (int)std::min(fit, kDefaultRows);
        }
    }
    p->init(s, code_object, code_size, nconst, TFK_EXTREMA_COUNT, 2);
    p->nblk = (int)tf_solver::cdiv(s->L1.P, 256);
    for (auto& exp : p->obs) {
        Extrema& ex = *exp;
        ex.counts.alloc(((size_t)s->nsys * p->nblk * 256 + 1) / 2, p->bytes);
        ex.sums.alloc(((size_t)s->nsys * p->nblk + 1) / 2, p->bytes);
        ex.ring.alloc(p->bytes);
    }
    *out = p.release();
    TF_API_END
}

void tf_extrema_destroy(tf_extrema* p) { delete p; }

int tf_extrema_set_consts(tf_extrema* p, const double* values, int32_t nconst) {
    TF_API_BEGIN
    require(p && (values || nconst == 0), "null argument");
    p->set_consts("tf_extrema", values, nconst);
    TF_API_END
}

int tf_extrema_set_x(tf_extrema* p, const double* x) {
    TF_API_BEGIN
    require(p && x, "null argument");
    p->set_x(x);
    TF_API_END
}

int tf_extrema_record(tf_extrema* p, int32_t which, int32_t slot) {
    TF_API_BEGIN
    require(p, "null extrema set");
    require(which >= 0 && which < (int)p->obs.size(), "tf_extrema_record: no such observer");
    tf_solver* s = p->solver;
    Extrema& ex = *p->obs[which];
    const int row = ex.ring.next_row(s->stream);
    TfExtremaArgs a;
    std::memset(&a, 0, sizeof a);
    static_cast<TfNodeArgs&>(a) = p->node_args(slot);
    a.which = ex.expr;
    a.kind = ex.kind;
    a.max_count = ex.max_count;
    a.nblk = p->nblk;
    a.row = row;
    a.capacity = ex.ring.capacity;
    a.threshold = ex.threshold;
    a.counts = (int*)ex.counts.p;
    a.sums = (int*)ex.sums.p;
    a.ring = ex.ring.ring.p;
    p->launch(TFK_EXTREMA_COUNT, (unsigned)(s->nsys * p->nblk), 1, 256, &a, sizeof a);
    p->launch(TFK_EXTREMA_WRITE, (unsigned)(s->nsys * p->nblk), 1, 256, &a, sizeof a);
    ++ex.ring.on_device;
    TF_API_END
}

int tf_extrema_fetch(tf_extrema* p, int32_t which, double* out, int64_t max_rows, int64_t* rows) {
    TF_API_BEGIN
    require(p && rows && (out || max_rows == 0), "null argument");
    require(which >= 0 && which < (int)p->obs.size(), "tf_extrema_fetch: no such observer");
    p->obs[which]->ring.fetch(p->solver->stream, out, max_rows, rows);
    TF_API_END
}

int tf_extrema_pending(tf_extrema* p, int32_t which, int64_t* rows) {
    TF_API_BEGIN
    require(p && rows, "null argument");
    require(which >= 0 && which < (int)p->obs.size(), "tf_extrema_pending: no such observer");
    *rows = p->obs[which]->ring.pending();
    TF_API_END
}

}  // extern "C"
