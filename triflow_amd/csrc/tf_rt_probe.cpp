// Host runtime of libtriflow_hip: device probes (tf_probe_*).  A probe set is a second code object of
// the solver's model -- the model's translation unit plus the generated probe block (codegen.lower_probes)
// -- of which only tfk_probe_partial / tfk_probe_final are launched, on the solver's stream, on one of
// its state slots.  The rows go into a ring in device memory; the host waits only when the ring is full
// (one copy of all of it) and when the caller fetches.
#include "tf_solver.h"

struct tf_probe {
    tf_solver* solver = nullptr;
    tfb::Module* module = nullptr;
    int nprobe = 0, capacity = 0, nhc = 0, nblk = 0, nseg = 0;
    int64_t bytes = 0;
    DevBuf hc, xplane, partial, ends, ring;    // ring: [0] row cursor + arrivals (2 ints), then the rows
    bool own_x = false;                        // the solver holds no x plane (its model does not read x)
    int on_device = 0;                         // rows queued since the ring was last emptied (host mirror)
    std::vector<double> host_rows;             // rows drained but not fetched yet, [row][nsys][nprobe]
    size_t row_size() const { return (size_t)solver->nsys * nprobe; }
    ~tf_probe() { if (module) tfb::module_unload(module); }

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

namespace {
void probe_launch(tf_probe* p, int kernel, unsigned gx, unsigned gy, const TfProbeArgs& a) {
    tf_solver* s = p->solver;
    if ((s->timing >> kernel) & 1ull) {          // (timed like the solver's own launches: tf_timing_get)
        tf_solver::Stamp st{kernel, s->get_event(), s->get_event()};
        tfb::launch_timed(p->module, kernel, gx, gy, 256, &a, sizeof(a), s->stream, st.a, st.b);
        s->stamps.push_back(st);
    } else {
        tfb::launch(p->module, kernel, gx, gy, 256, &a, sizeof(a), s->stream);
    }
}
}  // namespace

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
    p->solver = s;
    p->nprobe = nprobe;
    p->capacity = capacity;
    p->nhc = nconst;
    p->nblk = (int)tf_solver::cdiv(s->L1.P, 256);
    p->nseg = (int)tf_solver::cdiv(s->L1.M, TF_PROBE_SEG);
    p->module = tfb::module_load(code_object, code_size);
    const int nsys = s->nsys;
    p->hc.alloc((size_t)std::max(nconst, 1) * nsys, p->bytes);
    // x of the nodes (argmax / argmin, probes that read x): the solver's plane when its model reads x
    // (bound with the other inputs, tf_set_x), else a plane of the probe's own (tf_probe_set_x)
    p->own_x = !s->spec.uses_x;
    if (p->own_x) p->xplane.alloc((size_t)s->L1.plane, p->bytes);
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
    require(nconst == p->nhc, "tf_probe_set_consts: constant count differs from tf_probe_create");
    const int nsys = p->solver->nsys;
    std::vector<double> t((size_t)std::max(nconst, 1) * nsys, 0.0);    // [nsys][nconst] -> [nconst][nsys]
    for (int e = 0; e < nsys; ++e)
        for (int k = 0; k < nconst; ++k) t[(size_t)k * nsys + e] = values[(size_t)e * nconst + k];
    tfb::h2d(p->hc.p, t.data(), t.size() * sizeof(double), p->solver->stream);
    TF_API_END
}

int tf_probe_set_x(tf_probe* p, const double* x) {
    TF_API_BEGIN
    require(p && x, "null argument");
    if (p->own_x) p->solver->upload_planes(x, p->xplane.p, 1);
    TF_API_END
}

int tf_probe_record(tf_probe* p, int32_t slot) {
    TF_API_BEGIN
    require(p, "null probe");
    tf_solver* s = p->solver;
    if (p->on_device == p->capacity) p->drain();
    TfProbeArgs a;
    std::memset(&a, 0, sizeof a);
    a.L = s->L1;
    a.fields = s->st(slot);
    a.helpers = s->helpers.p;
    a.parvec = s->parvec.p;
    a.parsca = s->parsca.p;
    a.dx = s->dx.p;
    a.xcoord = p->own_x ? p->xplane.p : s->xcoord.p;
    a.hc = p->hc.p;
    a.partial = p->partial.p;
    a.ends = p->ends.p;
    a.nblk = p->nblk;
    a.nseg = p->nseg;
    a.capacity = p->capacity;
    a.cursor = (int*)p->ring.p;
    a.ring = p->ring.p + 1;
    probe_launch(p, TFK_PROBE_PARTIAL, (unsigned)(s->nsys * p->nblk), (unsigned)p->nseg, a);
    probe_launch(p, TFK_PROBE_FINAL, (unsigned)s->nsys, 1, a);
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
