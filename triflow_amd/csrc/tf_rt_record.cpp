// Host runtime of libtriflow_hip: device recorders (tf_record_*).  A recorder set is one more code object
// of the solver's model -- the model's generated body, the generated record block (codegen.lower_records)
// and tf_record.h -- that holds tfk_record, launched on the solver's stream, on one of its state slots
// (tf_observer, tf_solver.h: what the recorders share with the other observers): one launch per recorder
// that is due, one row [nsys][ncols] per launch.
//
// The rows of a recorder go into a ring of two halves in device memory, counted on the host and copied
// half by half on the recorder set's copy stream while the records go on (HalfRing, tf_solver.h).
#include "tf_solver.h"

namespace {
struct Recorder {
    int expr = 0, pool = 0, start = 0, stop = 0, step = 1, ncols = 0, split = 1, part = 1, nblk = 1;
    HalfRing ring;                             // a row: nsys * ncols doubles
};
}  // namespace

struct tf_record : tf_observer {
    tfb::Stream* copy = nullptr;
    std::vector<std::unique_ptr<Recorder>> recs;

    ~tf_record() {
        try { if (copy) tfb::stream_sync(copy); } catch (...) {}
        recs.clear();
        if (copy) tfb::stream_destroy(copy);
    }
};

extern "C" {

int tf_record_create(tf_solver* s, const void* code_object, size_t code_size, int32_t nrec,
                     const int32_t* geometry, int32_t nconst, tf_record** out) {
    TF_API_BEGIN
    require(s && out && geometry && code_object, "null argument");
    require(nrec >= 1 && nrec <= 64, "tf_record_create: 1 ... 64 recorders");
    require(nconst >= 0, "tf_record_create: bad constant count");
    std::unique_ptr<tf_record> p(new tf_record());
    const int nsys = s->nsys, N = s->L1.N;
    for (int k = 0; k < nrec; ++k) {
        const int32_t* g = geometry + 6 * k;
        p->recs.emplace_back(new Recorder());
        Recorder& r = *p->recs[k];
        r.expr = g[0]; r.pool = g[1]; r.start = g[2]; r.stop = g[3]; r.step = g[4];
        require(r.expr >= 0 && r.expr < nrec, "tf_record_create: no such expression");
        require(r.pool >= TF_REC_SAMPLE && r.pool <= TF_REC_MEAN, "tf_record_create: unknown pool");
        require(r.step >= 1 && r.start >= 0 && r.start < r.stop && r.stop <= N,
                "tf_record_create: the window of nodes is empty or leaves the system");
        require(g[5] >= 2, "tf_record_create: a ring has two rows at least (one per half)");
        r.ncols = (int)tf_solver::cdiv(r.stop - r.start, r.step);
        if (r.pool != TF_REC_SAMPLE)           // up to 8 nodes per thread, `split` (a power of two) threads per bin
            while (r.split < TF_REC_BLOCK && r.split * 8 < r.step) r.split *= 2;
        r.part = r.pool == TF_REC_SAMPLE ? 1 : (int)tf_solver::cdiv(r.step, r.split);
        r.nblk = (int)tf_solver::cdiv(r.ncols, TF_REC_BLOCK / r.split);
        r.ring.half = g[5] / 2;
        r.ring.row = (size_t)nsys * r.ncols;
    }
    p->init(s, code_object, code_size, nconst, TFK_RECORD, 1);
    p->copy = tfb::stream_create();
    for (auto& r : p->recs) r->ring.alloc(p->bytes);
    *out = p.release();
    TF_API_END
}

void tf_record_destroy(tf_record* p) { delete p; }

int tf_record_set_consts(tf_record* p, const double* values, int32_t nconst) {
    TF_API_BEGIN
    require(p && (values || nconst == 0), "null argument");
    p->set_consts("tf_record", values, nconst);
    TF_API_END
}

int tf_record_set_x(tf_record* p, const double* x) {
    TF_API_BEGIN
    require(p && x, "null argument");
    p->set_x(x);
    TF_API_END
}

int tf_record_record(tf_record* p, int32_t which, int32_t slot) {
    TF_API_BEGIN
    require(p, "null recorder");
    require(which >= 0 && which < (int)p->recs.size(), "tf_record_record: no such recorder");
    tf_solver* s = p->solver;
    Recorder& r = *p->recs[which];
    const int row = r.ring.begin_row(s->stream);
    TfRecordArgs a;
    std::memset(&a, 0, sizeof a);
    static_cast<TfNodeArgs&>(a) = p->node_args(slot);
    a.which = r.expr;
    a.pool = r.pool; a.start = r.start; a.stop = r.stop; a.step = r.step; a.ncols = r.ncols;
    a.split = r.split; a.part = r.part; a.nblk = r.nblk;
    a.row = row;
    a.capacity = 2 * r.ring.half;
    a.ring = r.ring.dev.p;
    p->launch(TFK_RECORD, (unsigned)(s->nsys * r.nblk), 1, TF_REC_BLOCK, &a, sizeof a);
    r.ring.end_row(s->stream, p->copy);
    TF_API_END
}

int tf_record_fetch(tf_record* p, int32_t which, double* out, int64_t max_rows, int64_t* rows) {
    TF_API_BEGIN
    require(p && rows && (out || max_rows == 0), "null argument");
    require(which >= 0 && which < (int)p->recs.size(), "tf_record_fetch: no such recorder");
    p->recs[which]->ring.fetch(p->solver->stream, p->copy, out, max_rows, rows);
    TF_API_END
}

int tf_record_pending(tf_record* p, int32_t which, int64_t* rows) {
    TF_API_BEGIN
    require(p && rows, "null argument");
    require(which >= 0 && which < (int)p->recs.size(), "tf_record_pending: no such recorder");
    *rows = p->recs[which]->ring.pending();
    TF_API_END
}

}  // extern "C"
