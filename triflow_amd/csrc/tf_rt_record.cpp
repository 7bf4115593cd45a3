// Host runtime of libtriflow_hip: device recorders (tf_record_*).  A recorder set is one more code object
// of the solver's model -- the model's generated body, the generated record block (codegen.lower_records)
// and tf_record.h -- that holds tfk_record, launched on the solver's stream, on one of its state slots
// (tf_observer, tf_solver.h: what the recorders share with the other observers): one launch per recorder
// that is due, one row [nsys][ncols] per launch.
//
// The rows of a recorder go into a ring of two halves in device memory.  When a half is full, an event on
// the solver's stream lets the recorder's copy stream move it into a page-locked buffer of that half
// while the records go on into the other half; before a half is written again the solver's stream waits
// (a stream-side wait) for the copy of it.  The host waits in fetch, and where the copy of a half needs a
// page-locked buffer whose rows it has not taken yet -- a copy queued two halves earlier.  Buffers,
// streams and events are made at create; rows taken but not fetched grow one vector per recorder.
#include "tf_solver.h"

// Back ends without asynchronous copies (tf_backend.h): the same calls without the overlap.
namespace tfb {
__attribute__((weak)) void* host_alloc(size_t bytes) { return std::malloc(bytes ? bytes : 8); }
__attribute__((weak)) void host_free(void* p) { std::free(p); }
__attribute__((weak)) void d2h_async(void* dst, const void* src, size_t bytes, Stream* s) { d2h(dst, src, bytes, s); }
__attribute__((weak)) void stream_wait_event(Stream*, Event*) {}
__attribute__((weak)) void event_sync(Event*) {}
}  // namespace tfb

namespace {
struct Ring {
    int expr = 0, pool = 0, start = 0, stop = 0, step = 1, ncols = 0, split = 1, part = 1, nblk = 1;
    int half = 1;                              // rows of one half
    size_t row = 0;                            // doubles of one row: nsys * ncols
    DevBuf dev;                                // [0]: row cursor + arrivals (2 ints), then 2 * half rows
    double* pinned[2] = {nullptr, nullptr};
    tfb::Event* full[2] = {nullptr, nullptr};  // on the solver's stream: the rows of half h are written
    tfb::Event* copied[2] = {nullptr, nullptr};   // on the copy stream: half h is in pinned[h]
    int64_t head = 0;                          // rows recorded so far (row head % (2 * half) is next)
    int lo[2] = {0, 0};                        // rows at the start of half h that were fetched from a part-filled half
    int flying[2] = {0, 0};                    // rows of pinned[h] (copied or on their way) not taken yet
    bool guard[2] = {false, false};            // the next write into half h has to wait for copied[h]
    std::vector<double> rows;                  // taken, not fetched
    double* rows_of(int h, int r) const { return dev.p + 1 + ((size_t)h * half + r) * row; }
};
}  // namespace

struct tf_record : tf_observer {
    tfb::Stream* copy = nullptr;
    std::vector<std::unique_ptr<Ring>> rings;

    ~tf_record() {
        try { if (copy) tfb::stream_sync(copy); } catch (...) {}
        for (auto& r : rings)
            for (int h = 0; h < 2; ++h) {
                tfb::host_free(r->pinned[h]);
                tfb::event_destroy(r->full[h]);
                tfb::event_destroy(r->copied[h]);
            }
        if (copy) tfb::stream_destroy(copy);
    }

    // rows [lo, lo + n) of half h to pinned[h], behind what the solver's stream has queued so far
    void queue_copy(Ring& r, int h, int lo, int n) {
        tfb::event_record(r.full[h], solver->stream);
        tfb::stream_wait_event(copy, r.full[h]);
        tfb::d2h_async(r.pinned[h], r.rows_of(h, lo), (size_t)n * r.row * sizeof(double), copy);
        tfb::event_record(r.copied[h], copy);
        r.flying[h] = n;
    }
    // the rows of pinned[h] to r.rows (waits for their copy)
    void take(Ring& r, int h) {
        if (r.flying[h] == 0) return;
        tfb::event_sync(r.copied[h]);
        r.rows.insert(r.rows.end(), r.pinned[h], r.pinned[h] + (size_t)r.flying[h] * r.row);
        r.flying[h] = 0;
    }
    // every recorded row to r.rows, oldest first
    void drain(Ring& r) {
        const int h = (int)((r.head / r.half) % 2), fill = (int)(r.head % r.half);
        take(r, h);                            // (the copy of this half's last round is the older one)
        take(r, 1 - h);
        if (fill > r.lo[h]) {
            queue_copy(r, h, r.lo[h], fill - r.lo[h]);
            take(r, h);
            r.lo[h] = fill;
        }
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
        p->rings.emplace_back(new Ring());
        Ring& r = *p->rings[k];
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
        r.half = g[5] / 2;
        r.row = (size_t)nsys * r.ncols;
    }
    p->init(s, code_object, code_size, nconst, TFK_RECORD, 1);
    p->copy = tfb::stream_create();
    for (auto& rp : p->rings) {
        Ring& r = *rp;
        r.dev.alloc(1 + 2 * (size_t)r.half * r.row, p->bytes);         // (zero-filled: cursor 0)
        for (int h = 0; h < 2; ++h) {
            r.pinned[h] = (double*)tfb::host_alloc((size_t)r.half * r.row * sizeof(double));
            r.full[h] = tfb::event_create();
            r.copied[h] = tfb::event_create();
        }
    }
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
    require(which >= 0 && which < (int)p->rings.size(), "tf_record_record: no such recorder");
    tf_solver* s = p->solver;
    Ring& r = *p->rings[which];
    const int h = (int)((r.head / r.half) % 2);
    if (r.head % r.half == 0 && r.guard[h]) {          // first row of a half that was copied: after its copy
        tfb::stream_wait_event(s->stream, r.copied[h]);
        r.guard[h] = false;
    }
    TfRecordArgs a;
    std::memset(&a, 0, sizeof a);
    static_cast<TfNodeArgs&>(a) = p->node_args(slot);
    a.which = r.expr;
    a.pool = r.pool; a.start = r.start; a.stop = r.stop; a.step = r.step; a.ncols = r.ncols;
    a.split = r.split; a.part = r.part; a.nblk = r.nblk;
    a.capacity = 2 * r.half;
    a.cursor = (int*)r.dev.p;
    a.ring = r.dev.p + 1;
    p->launch(TFK_RECORD, (unsigned)(s->nsys * r.nblk), 1, TF_REC_BLOCK, &a, sizeof a);
    ++r.head;
    if (r.head % r.half == 0) {                        // half h is full: its copy, while the other half fills
        p->take(r, h);                                 // (rows of this half's last round still in pinned[h])
        p->queue_copy(r, h, r.lo[h], r.half - r.lo[h]);
        r.lo[h] = 0;
        r.guard[h] = true;
    }
    TF_API_END
}

int tf_record_fetch(tf_record* p, int32_t which, double* out, int64_t max_rows, int64_t* rows) {
    TF_API_BEGIN
    require(p && rows && (out || max_rows == 0), "null argument");
    require(which >= 0 && which < (int)p->rings.size(), "tf_record_fetch: no such recorder");
    Ring& r = *p->rings[which];
    const int h = (int)((r.head / r.half) % 2), fill = (int)(r.head % r.half);
    const int64_t taken = (int64_t)(r.rows.size() / r.row);
    if (max_rows >= taken + r.flying[0] + r.flying[1] + fill - r.lo[h]) {
        // everything fits: the rows of the page-locked buffers go straight to the caller, oldest first
        double* at = out;
        auto put = [&](const double* src, size_t n) { if (n) std::memcpy(at, src, n * r.row * sizeof(double)); at += n * r.row; };
        put(r.rows.data(), (size_t)taken);
        r.rows.clear();
        for (int hh : {h, 1 - h}) {                    // (the copy of this half's last round is the older one)
            if (r.flying[hh] == 0) continue;
            tfb::event_sync(r.copied[hh]);
            put(r.pinned[hh], (size_t)r.flying[hh]);
            r.flying[hh] = 0;
        }
        if (fill > r.lo[h]) {
            p->queue_copy(r, h, r.lo[h], fill - r.lo[h]);
            tfb::event_sync(r.copied[h]);
            put(r.pinned[h], (size_t)r.flying[h]);
            r.flying[h] = 0;
            r.lo[h] = fill;
        }
        *rows = (int64_t)((at - out) / (int64_t)r.row);
        return 0;
    }
    p->drain(r);
    const int64_t have = (int64_t)(r.rows.size() / r.row);
    const int64_t n = std::min<int64_t>(have, std::max<int64_t>(max_rows, 0));
    if (n) std::memcpy(out, r.rows.data(), (size_t)n * r.row * sizeof(double));
    r.rows.erase(r.rows.begin(), r.rows.begin() + (size_t)n * r.row);
    *rows = n;
    TF_API_END
}

int tf_record_pending(tf_record* p, int32_t which, int64_t* rows) {
    TF_API_BEGIN
    require(p && rows, "null argument");
    require(which >= 0 && which < (int)p->rings.size(), "tf_record_pending: no such recorder");
    const Ring& r = *p->rings[which];
    const int h = (int)((r.head / r.half) % 2);
    *rows = (int64_t)(r.rows.size() / r.row) + r.flying[0] + r.flying[1] + (r.head % r.half) - r.lo[h];
    TF_API_END
}

}  // extern "C"
