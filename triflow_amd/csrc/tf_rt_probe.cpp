// Host runtime of libtriflow_hip: device probes (tf_probe_*).  A probe set is a second code object of
// the solver's model -- the model's generated body, the generated probe block (codegen.lower_probes) and
// tf_probe.h -- that holds tfk_probe_partial / tfk_probe_final, launched on the solver's stream, on one of
// its state slots (tf_observer, tf_solver.h: what the probes share with the other observers).  The rows go into
// a ring in device memory, counted on the host (RowRing, tf_solver.h).
#include "tf_solver.h"

struct tf_probe : tf_observer {
    int nprobe = 0, nblk = 0, nseg = 0;
    DevBuf partial, ends;
    RowRing ring;                              // a row: nsys * nprobe doubles
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
    p->nblk = (int)tf_solver::cdiv(s->L1.P, 256);
    p->nseg = (int)tf_solver::cdiv(s->L1.M, TF_PROBE_SEG);
    const int nsys = s->nsys;
    p->partial.alloc((size_t)nsys * nprobe * p->nseg * p->nblk * 2, p->bytes);
    p->ends.alloc((size_t)nsys * nprobe * 2, p->bytes);
    p->ring.capacity = capacity;
    p->ring.row = (size_t)nsys * nprobe;
    p->ring.alloc(p->bytes);
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
    const int row = p->ring.next_row(s->stream);
    TfProbeArgs a;
    std::memset(&a, 0, sizeof a);
    static_cast<TfNodeArgs&>(a) = p->node_args(slot);
    a.partial = p->partial.p;
    a.ends = p->ends.p;
    a.nblk = p->nblk;
    a.nseg = p->nseg;
    a.row = row;
    a.capacity = p->ring.capacity;
    a.ring = p->ring.ring.p;
    p->launch(TFK_PROBE_PARTIAL, (unsigned)(s->nsys * p->nblk), (unsigned)p->nseg, 256, &a, sizeof a);
    p->launch(TFK_PROBE_FINAL, (unsigned)s->nsys, 1, 256, &a, sizeof a);
    ++p->ring.on_device;
    TF_API_END
}

int tf_probe_fetch(tf_probe* p, double* out, int64_t max_rows, int64_t* rows) {
    TF_API_BEGIN
    require(p && rows && (out || max_rows == 0), "null argument");
    p->ring.fetch(p->solver->stream, out, max_rows, rows);
    TF_API_END
}

int tf_probe_pending(tf_probe* p, int64_t* rows) {
    TF_API_BEGIN
    require(p && rows, "null argument");
    *rows = p->ring.pending();
    TF_API_END
}

}  // extern "C"
