// Host runtime of libtriflow_hip: device probes (tf_probe_*).  A probe set is a second code object of
// the solver's model -- the model's generated body, the generated probe block (codegen.lower_probes) and
// tf_probe.h -- that holds tfk_probe_partial / tfk_probe_final, launched on the solver's stream, on one of
// its state slots (tf_observer, tf_solver.h: what the probes share with the other observers).  The rows go into
// a ring in device memory; the host waits only when the ring is full (one copy of all of it) and when the
// caller fetches.
#include "tf_solver.h"

struct tf_probe : tf_observer {
    int nprobe = 0, capacity = 0, nblk = 0, nseg = 0;
    DevBuf partial, ends, ring;                // ring: [0] row cursor + arrivals (2 ints), then the rows
    int on_device = 0;                         // rows queued since the ring was last emptied (host mirror)
    std::vector<double> host_rows;             // rows drained but not fetched yet, [row][nsys][nprobe]
    size_t row_size() const { return (size_t)solver->nsys * nprobe; }

    // the ring's rows to host_rows, one copy; the cursor goes back to row 0 (queued on the stream)
    void drain() {
        if (on_device == 0) return;
        const size_t n = 1 + (size_t)on_device * row_size();
        std::vector<double> buf(n);
        tfb::d2h(buf.data(), ring.p, n * sizeof(double), solver->stream);
        int hdr[2];
        std::memcpy(hdr, buf.data(), sizeof hdr);
        if (hdr[0] != on_device)
            throw std::runtime_error("tf_probe: the ring holds " + std::to_string(hdr[0]) + " rows, " +
                                     std::to_string(on_device) + " were recorded");
        host_rows.insert(host_rows.end(), buf.begin() + 1, buf.end());
        tfb::memset0(ring.p, sizeof(double), solver->stream);
        on_device = 0;
    }
};

extern "C" {

int tf_probe_create(tf_solver* s, const void* code_object, size_t code_size, int32_t nprobe,
                    const int32_t* kinds, int32_t nconst, int32_t capacity, tf_probe** out) {
    TF_API_BEGIN
    require(s && out && kinds, "null argument");
    require(nprobe >= 1 && nprobe <= 64, "tf_probe_create: 1 ... 64 probes");
    require(nconst >= 0 && capacity >= 1, "tf_probe_create: bad constant count / capacity");
    for (int k = 0; k < nprobe; ++k)
        require(kinds[k] >= 0 && kinds[k] < TF_PROBE_KINDS, "tf_probe_create: unknown reduction");
    std::unique_ptr<tf_probe> p(new tf_probe());
    p->init(s, code_object, code_size, nconst, TFK_PROBE_PARTIAL, 2);
    p->nprobe = nprobe;
    p->capacity = capacity;
    p->nblk = (int)tf_solver::cdiv(s->L1.P, 256);
    p->nseg = (int)tf_solver::cdiv(s->L1.M, TF_PROBE_SEG);
    const int nsys = s->nsys;
    p->partial.alloc((size_t)nsys * nprobe * p->nseg * p->nblk * 2, p->bytes);
    p->ends.alloc((size_t)nsys * nprobe * 2, p->bytes);
    p->ring.alloc(1 + (size_t)capacity * nsys * nprobe, p->bytes);      // (zero-filled: cursor 0)
    *out = p.release();
    TF_API_END
}

void tf_probe_destroy(tf_probe* p) { delete p; }

int tf_probe_set_consts(tf_probe* p, const double* values, int32_t nconst) {
    TF_API_BEGIN
    require(p && (values || nconst == 0), "null argument");
    p->set_consts("tf_probe", values, nconst);
    TF_API_END
}

int tf_probe_set_x(tf_probe* p, const double* x) {
    TF_API_BEGIN
    require(p && x, "null argument");
    p->set_x(x);
    TF_API_END
}

int tf_probe_record(tf_probe* p, int32_t slot) {
    TF_API_BEGIN
    require(p, "null probe");
    tf_solver* s = p->solver;
    if (p->on_device == p->capacity) p->drain();
    TfProbeArgs a;
    std::memset(&a, 0, sizeof a);
    static_cast<TfNodeArgs&>(a) = p->node_args(slot);
    a.partial = p->partial.p;
    a.ends = p->ends.p;
    a.nblk = p->nblk;
    a.nseg = p->nseg;
    a.capacity = p->capacity;
    a.cursor = (int*)p->ring.p;
    a.ring = p->ring.p + 1;
    p->launch(TFK_PROBE_PARTIAL, (unsigned)(s->nsys * p->nblk), (unsigned)p->nseg, 256, &a, sizeof a);
    p->launch(TFK_PROBE_FINAL, (unsigned)s->nsys, 1, 256, &a, sizeof a);
    ++p->on_device;
    TF_API_END
}

int tf_probe_fetch(tf_probe* p, double* out, int64_t max_rows, int64_t* rows) {
    TF_API_BEGIN
    require(p && rows && (out || max_rows == 0), "null argument");
    p->drain();
    const size_t rs = p->row_size();
    const int64_t have = (int64_t)(p->host_rows.size() / rs);
    const int64_t n = std::min<int64_t>(have, std::max<int64_t>(max_rows, 0));
    if (n) std::memcpy(out, p->host_rows.data(), (size_t)n * rs * sizeof(double));
    p->host_rows.erase(p->host_rows.begin(), p->host_rows.begin() + (size_t)n * rs);
    *rows = n;
    TF_API_END
}

int tf_probe_pending(tf_probe* p, int64_t* rows) {
    TF_API_BEGIN
    require(p && rows, "null argument");
    *rows = p->on_device + (int64_t)(p->host_rows.size() / p->row_size());
    TF_API_END
}

}  // extern "C"
