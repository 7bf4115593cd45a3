// Host runtime of libtriflow_hip: device statistics (tf_stat_*).  A statistic set is one more code object
// of the solver's model -- the model's generated body, the generated statistic block
// (codegen.lower_statistics) and tf_stat.h -- that holds tfk_stat, launched on the solver's stream, on one
// of its state slots (tf_observer, tf_solver.h: what the statistics share with the other observers): one
// launch per statistic that is due.
//
// A statistic owns one or two accumulator planes (tf_stat_planes) in the solver's partition-interleaved
// layout; a launch folds one sample into them.  The number of the sample and its time are the caller's
// and travel by value: nothing of a statistic but its planes lives on the device, so an update never
// waits, a reset is the caller counting from 1 again, and the planes come and go in natural order through
// the solver's own permutation (fetch, load: a set that moves to another solver takes them along).
#include "tf_solver.h"

namespace {
struct Acc {
    int expr = 0, kind = 0, planes = 1;
    DevBuf dev;                                // [planes] planes
};
}  // namespace

struct tf_stat : tf_observer {
    int nblk = 0, nseg = 0;
    std::vector<std::unique_ptr<Acc>> accs;
};

extern "C" {

int tf_stat_create(tf_solver* s, const void* code_object, size_t code_size, int32_t nstat,
                   const int32_t* geometry, int32_t nconst, tf_stat** out) {
    TF_API_BEGIN
    require(s && out && geometry && code_object, "null argument");
    require(nstat >= 1 && nstat <= 64, "tf_stat_create: 1 ... 64 statistics");
    require(nconst >= 0, "tf_stat_create: bad constant count");
    std::unique_ptr<tf_stat> p(new tf_stat());
    int nexpr = 0;
    for (int k = 0; k < nstat; ++k) {
        p->accs.emplace_back(new Acc());
        Acc& a = *p->accs[k];
        a.expr = geometry[2 * k];
        a.kind = geometry[2 * k + 1];
        tf_observer::require_numbered_in_order(
            a.expr, nexpr, "tf_stat_create: expressions are numbered in the order the statistics first use them");
        require(a.kind >= 0 && a.kind < TF_STAT_KINDS, "tf_stat_create: unknown kind of statistic");
        a.planes = tf_stat_planes(a.kind);
    }
    p->init(s, code_object, code_size, nconst, TFK_STAT, 1);
    p->nblk = (int)tf_solver::cdiv(s->L1.P, 256);
    p->nseg = (int)tf_solver::cdiv(s->L1.M, TF_PROBE_SEG);
    for (auto& a : p->accs) a->dev.alloc((size_t)a->planes * s->L1.plane, p->bytes);
    *out = p.release();
    TF_API_END
}

void tf_stat_destroy(tf_stat* p) { delete p; }

int tf_stat_set_consts(tf_stat* p, const double* values, int32_t nconst) {
    TF_API_BEGIN
    require(p && (values || nconst == 0), "null argument");
    p->set_consts("tf_stat", values, nconst);
    TF_API_END
}

int tf_stat_set_x(tf_stat* p, const double* x) {
    TF_API_BEGIN
    require(p && x, "null argument");
    p->set_x(x);
    TF_API_END
}

int tf_stat_update(tf_stat* p, int32_t which, int32_t slot, int64_t k, double t) {
    TF_API_BEGIN
    require(p, "null statistic");
    require(which >= 0 && which < (int)p->accs.size(), "tf_stat_update: no such statistic");
    require(k >= 1, "tf_stat_update: samples are counted from 1");
    tf_solver* s = p->solver;
    Acc& acc = *p->accs[which];
    TfStatArgs a;
    std::memset(&a, 0, sizeof a);
    static_cast<TfNodeArgs&>(a) = p->node_args(slot);
    a.which = acc.expr;
    a.kind = acc.kind;
    a.nblk = p->nblk;
    a.nseg = p->nseg;
    a.k = (double)k;
    a.t = t;
    a.acc = acc.dev.p;
    p->launch(TFK_STAT, (unsigned)(s->nsys * p->nblk), (unsigned)p->nseg, 256, &a, sizeof a);
    TF_API_END
}

int tf_stat_planes_of(tf_stat* p, int32_t which, int32_t* planes) {
    TF_API_BEGIN
    require(p && planes, "null argument");
    require(which >= 0 && which < (int)p->accs.size(), "tf_stat_planes_of: no such statistic");
    *planes = p->accs[which]->planes;
    TF_API_END
}

int tf_stat_fetch(tf_stat* p, int32_t which, double* out) {
    TF_API_BEGIN
    require(p && out, "null argument");
    require(which >= 0 && which < (int)p->accs.size(), "tf_stat_fetch: no such statistic");
    const Acc& acc = *p->accs[which];
    p->solver->download_planes(acc.dev.p, out, acc.planes);
    TF_API_END
}

int tf_stat_load(tf_stat* p, int32_t which, const double* in) {
    TF_API_BEGIN
    require(p && in, "null argument");
    require(which >= 0 && which < (int)p->accs.size(), "tf_stat_load: no such statistic");
    Acc& acc = *p->accs[which];
    p->solver->upload_planes(in, acc.dev.p, acc.planes);
    TF_API_END
}

}  // extern "C"
