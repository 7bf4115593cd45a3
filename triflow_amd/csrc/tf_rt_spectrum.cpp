// Host runtime of libtriflow_hip: device spectra (tf_spectrum_*).  A spectrum set is one more code object
// of the solver's model -- the model's generated body, the generated spectrum block (codegen.lower_spectra)
// and tf_spectrum.h -- that holds tfk_spectrum_partial / tfk_spectrum_final, launched on the
// solver's stream, on one of its state slots (tf_observer, tf_solver.h: what the spectra share with the
// other observers): the two launches per spectrum that is due, one row [nsys][nmodes] of (re, im) pairs
// per record.
//
// A spectrum owns its modes (a device buffer: the code object does not know them), the partials of its
// workgroups and a ring of rows in device memory, counted on the host (RowRing, tf_solver.h).
#include "tf_solver.h"

namespace {
struct Spectrum {
    int expr = 0, nmodes = 0;
    DevBuf modes, partial;                     // modes: int32 [nmodes] in a buffer of doubles
    RowRing ring;                              // a row: nsys * nmodes * 2 doubles
};
}  // namespace

struct tf_spectrum : tf_observer {
    int nblk = 0, nseg = 0;
    std::vector<std::unique_ptr<Spectrum>> specs;
};

extern "C" {

int tf_spectrum_create(tf_solver* s, const void* code_object, size_t code_size, int32_t nspec,
                       const int32_t* geometry, int32_t nconst, tf_spectrum** out) {
    TF_API_BEGIN
    require(s && out && geometry && code_object, "null argument");
    require(nspec >= 1 && nspec <= 64, "tf_spectrum_create: 1 ... 64 spectra");
    require(nconst >= 0, "tf_spectrum_create: bad constant count");
    std::unique_ptr<tf_spectrum> p(new tf_spectrum());
    int nexpr = 0;
    for (int k = 0; k < nspec; ++k) {
        const int32_t* g = geometry + 3 * k;
        p->specs.emplace_back(new Spectrum());
        Spectrum& sp = *p->specs[k];
        sp.expr = g[0]; sp.nmodes = g[1]; sp.ring.capacity = g[2];
        tf_observer::require_numbered_in_order(
            sp.expr, nexpr, "tf_spectrum_create: expressions are numbered in the order the spectra first use them");
        require(sp.nmodes >= 1 && sp.nmodes <= TF_SPEC_MAX_MODES, "tf_spectrum_create: 1 ... 64 modes per spectrum");
        require(sp.ring.capacity >= 1, "tf_spectrum_create: a ring has one row at least");
    }
    p->init(s, code_object, code_size, nconst, TFK_SPECTRUM_PARTIAL, 2);
    p->nblk = (int)tf_solver::cdiv(s->L1.P, 256);
    p->nseg = (int)tf_solver::cdiv(s->L1.M, TF_PROBE_SEG);
    for (auto& spp : p->specs) {
        Spectrum& sp = *spp;
        sp.ring.row = (size_t)s->nsys * sp.nmodes * 2;
        sp.modes.alloc(((size_t)sp.nmodes + 1) / 2, p->bytes);          // (zero-filled: mode 0 until set_modes)
        sp.partial.alloc((size_t)s->nsys * sp.nmodes * p->nseg * p->nblk * 2, p->bytes);
        sp.ring.alloc(p->bytes);
    }
    *out = p.release();
    TF_API_END
}

void tf_spectrum_destroy(tf_spectrum* p) { delete p; }

int tf_spectrum_set_consts(tf_spectrum* p, const double* values, int32_t nconst) {
    TF_API_BEGIN
    require(p && (values || nconst == 0), "null argument");
    p->set_consts("tf_spectrum", values, nconst);
    TF_API_END
}

int tf_spectrum_set_x(tf_spectrum* p, const double* x) {
    TF_API_BEGIN
    require(p && x, "null argument");
    p->set_x(x);
    TF_API_END
}

int tf_spectrum_set_modes(tf_spectrum* p, int32_t which, const int32_t* modes, int32_t nmodes) {
    TF_API_BEGIN
    require(p && modes, "null argument");
    require(which >= 0 && which < (int)p->specs.size(), "tf_spectrum_set_modes: no such spectrum");
    Spectrum& sp = *p->specs[which];
    require(nmodes == sp.nmodes, "tf_spectrum_set_modes: mode count differs from tf_spectrum_create");
    const int N = p->solver->L1.N;
    for (int k = 0; k < nmodes; ++k)                   // (the kernels take m * g mod N in 64 bits: m <= N / 2)
        require(modes[k] >= 0 && modes[k] <= N / 2, "tf_spectrum_set_modes: a mode is 0 ... N / 2");
    tfb::h2d(sp.modes.p, modes, (size_t)nmodes * sizeof(int32_t), p->solver->stream);
    TF_API_END
}

int tf_spectrum_record(tf_spectrum* p, int32_t which, int32_t slot) {
    TF_API_BEGIN
    require(p, "null spectrum");
    require(which >= 0 && which < (int)p->specs.size(), "tf_spectrum_record: no such spectrum");
    tf_solver* s = p->solver;
    Spectrum& sp = *p->specs[which];
    const int row = sp.ring.next_row(s->stream);
    TfSpectrumArgs a;
    std::memset(&a, 0, sizeof a);
    static_cast<TfNodeArgs&>(a) = p->node_args(slot);
    a.which = sp.expr;
    a.nmodes = sp.nmodes;
    a.nblk = p->nblk;
    a.nseg = p->nseg;
    a.row = row;
    a.capacity = sp.ring.capacity;
    a.modes = (const int*)sp.modes.p;
    a.partial = sp.partial.p;
    a.ring = sp.ring.ring.p;
    p->launch(TFK_SPECTRUM_PARTIAL, (unsigned)(s->nsys * p->nblk), (unsigned)p->nseg, 256, &a, sizeof a);
    p->launch(TFK_SPECTRUM_FINAL, (unsigned)s->nsys, 1, 256, &a, sizeof a);
    ++sp.ring.on_device;
    TF_API_END
}

int tf_spectrum_fetch(tf_spectrum* p, int32_t which, double* out, int64_t max_rows, int64_t* rows) {
    TF_API_BEGIN
    require(p && rows && (out || max_rows == 0), "null argument");
    require(which >= 0 && which < (int)p->specs.size(), "tf_spectrum_fetch: no such spectrum");
    p->specs[which]->ring.fetch(p->solver->stream, out, max_rows, rows);
    TF_API_END
}

int tf_spectrum_pending(tf_spectrum* p, int32_t which, int64_t* rows) {
    TF_API_BEGIN
    require(p && rows, "null argument");
    require(which >= 0 && which < (int)p->specs.size(), "tf_spectrum_pending: no such spectrum");
    *rows = p->specs[which]->ring.pending();
    TF_API_END
}

}  // extern "C"
