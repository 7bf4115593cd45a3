// Host runtime of libtriflow_hip: device hooks (tf_hook_*).  A hook program is one more code object of the
// solver's model -- the model's generated body, the generated hook block (codegen.lower_hooks) and tf_hook.h
// -- that holds tfk_hook_window / tfk_hook_points.  Unlike the observers' kernels (tf_observer, tf_solver.h:
// what the hook shares with them -- the code object, the inputs of the node core, x and the host constants)
// these WRITE the state they run on: while a program is attached, tf_solver::apply_dirichlet runs it after
// the Dirichlet list, inside the step functions and so inside their captured graphs.
//
// The two kernels are not in the kernel table (tf_args.h).  They are looked up by name in the program's own
// code object when the handle is created (tfb::kernel_lookup) and launched through what the lookup
// returned, so they have no launch id, no bit of the timing mask and no line in tf_timing_get: a kernel
// trace times them.
//
// A program has two sets of host constants in device memory, for the call before the step and the call
// after it.  t is one of them (codegen.lower_hooks): a launch carries the address of a set and nothing of
// its contents, and tf_hook_set_consts uploads between the steps, so a replayed graph sees the new t.
#include "tf_solver.h"

namespace {
struct HookStatement { int kind = 0, var = 0, a = 0, b = 0, c = 0; };
// a maximal run of consecutive statements of one kind: one launch
struct HookRun {
    int kind = 0, first = 0, count = 0;
    // window runs: the chunks p0 ... p1 - 1 and the segments sg0 ... sg0 + nsg - 1 the union of the windows
    // touches (nsg == 0: every window of the run is empty, nothing is launched)
    int p0 = 0, p1 = 0, sg0 = 0, nsg = 0;
};
uint64_t g_hook_uid = 0;
}  // namespace

struct tf_hook : tf_observer {
    tfb::Function* fn_window = nullptr;      // tfk_hook_window, tfk_hook_points of the program's code object
    tfb::Function* fn_points = nullptr;
    std::vector<HookStatement> statements;
    std::vector<HookRun> runs;
    DevBuf hc_post;                          // the `after` set (tf_observer::hc is the `before` set)
    std::vector<double> consts, consts_post; // host mirrors
    double t_before = 0.0, t_after = 0.0;
    bool have_consts = false;
    uint64_t uid = 0;

    // chunk and row of natural node g (tf_locate of tf_layout.h)
    static void locate(const TfLayout& L, int g, int& p, int& i) {
        const int big = L.rem * (L.mbase + 1);
        if (g < big) { p = g / (L.mbase + 1); i = g - p * (L.mbase + 1); }
        else { const int h = g - big; p = L.rem + h / L.mbase; i = h - (h / L.mbase) * L.mbase; }
    }
    void plan_runs() {
        const TfLayout& L = solver->L1;
        for (size_t k = 0; k < statements.size(); ++k) {
            if (runs.empty() || runs.back().kind != statements[k].kind) {
                HookRun r;
                r.kind = statements[k].kind; r.first = (int)k;
                runs.push_back(r);
            }
            ++runs.back().count;
        }
        for (HookRun& r : runs) {
            if (r.kind != TF_HOOK_WINDOW) continue;
            int glo = L.N, ghi = -1;                   // first and last node any window of the run assigns
            for (int k = r.first; k < r.first + r.count; ++k) {
                const HookStatement& st = statements[k];
                if (st.b <= st.a) continue;
                glo = std::min(glo, st.a);
                ghi = std::max(ghi, st.a + (st.b - 1 - st.a) / st.c * st.c);
            }
            if (ghi < 0) continue;
            int plo, ilo, phi, ihi;
            locate(L, glo, plo, ilo);
            locate(L, ghi, phi, ihi);
            r.p0 = plo; r.p1 = phi + 1;
            // (several chunks: their rows from 0 to the longest chunk's last one; one chunk: its rows ilo ... ihi)
            const int rlo = plo == phi ? ilo : 0, rhi = plo == phi ? ihi : L.M - 1;
            r.sg0 = rlo / TF_PROBE_SEG;
            r.nsg = rhi / TF_PROBE_SEG - r.sg0 + 1;
        }
    }
    // the signature of what the program writes, per set: the program and the set (tf_solver::hook_sig adds
    // the upload count of the parameters as it stands when it is asked)
    void publish() {
        tf_solver* s = solver;
        if (s->prog != this) return;
        for (int post = 0; post < 2; ++post) {
            std::vector<double>& sig = post ? s->prog_sig_post : s->prog_sig;
            sig.assign(1, (double)uid);
            const std::vector<double>& c = post ? consts_post : consts;
            sig.insert(sig.end(), c.begin(), c.end());
        }
    }
    void run(double* fields, bool post) {
        tf_solver* s = solver;
        if (!have_consts) throw std::invalid_argument("tf_hook: set_consts before the program is applied");
        if (s->mode == tf_solver::TF_DRY) return;
        TfHookArgs a;
        std::memset(&a, 0, sizeof a);
        static_cast<TfNodeArgs&>(a) = node_args(0);
        a.fields = fields;
        a.out = fields;
        a.hc = post ? hc_post.p : hc.p;
        for (const HookRun& r : runs) {
            a.first = r.first; a.count = r.count;
            if (r.kind == TF_HOOK_POINT) {
                tfb::launch_function(fn_points, tf_solver::cdiv(s->nsys, 64), 1, 64, &a, sizeof a, s->stream);
                continue;
            }
            if (r.nsg == 0) continue;
            a.p0 = r.p0; a.p1 = r.p1; a.sg0 = r.sg0;
            a.nblk = (int)tf_solver::cdiv(r.p1 - r.p0, 256);
            tfb::launch_function(fn_window, (unsigned)(s->nsys * a.nblk), (unsigned)r.nsg, 256, &a, sizeof a, s->stream);
        }
    }
    static void apply_thunk(void* self, double* fields, bool post) { static_cast<tf_hook*>(self)->run(fields, post); }
    void detach() {
        tf_solver* s = solver;
        if (s->prog != this) return;
        s->drop_graphs();                             // (captured steps hold this program's launches)
        s->prog = nullptr; s->prog_apply = nullptr; s->prog_idem = false; s->prog_uid = 0;
        s->prog_sig.clear(); s->prog_sig_post.clear();
        s->slot_hook.clear();                         // (what the slots satisfied named this program)
    }
};

extern "C" {

int tf_hook_create(tf_solver* s, const void* code_object, size_t code_size, int32_t nstatement,
                   const int32_t* geometry, int32_t nconst, tf_hook** out) {
    TF_API_BEGIN
    require(s && out && geometry && code_object, "null argument");
    require(nstatement >= 1 && nstatement <= 256, "tf_hook_create: 1 ... 256 statements");
    require(nconst >= 0, "tf_hook_create: bad constant count");
    std::unique_ptr<tf_hook> p(new tf_hook());
    const int N = s->L1.N;
    for (int k = 0; k < nstatement; ++k) {
        const int32_t* g = geometry + 5 * k;
        HookStatement st;
        st.kind = g[0]; st.var = g[1]; st.a = g[2]; st.b = g[3]; st.c = g[4];
        require(st.kind == TF_HOOK_POINT || st.kind == TF_HOOK_WINDOW, "tf_hook_create: a statement is a point (0) or a window (1)");
        require(st.var >= 0 && st.var < s->spec.nvar, "tf_hook_create: the target is a dependent variable");
        if (st.kind == TF_HOOK_POINT)
            require(st.a >= 0 && st.a < N, "tf_hook_create: the node of a point statement is 0 ... N - 1");
        else
            require(st.c >= 1 && st.a >= 0 && st.a <= N && st.b >= 0 && st.b <= N,
                    "tf_hook_create: the window is slice.indices(N) with a step >= 1");
        p->statements.push_back(st);
    }
    p->init(s, code_object, code_size, nconst, 0, 0);
    p->fn_window = tfb::kernel_lookup(p->module, "tfk_hook_window");
    p->fn_points = tfb::kernel_lookup(p->module, "tfk_hook_points");
    p->hc_post.alloc((size_t)std::max(nconst, 1) * s->nsys, p->bytes);
    p->uid = ++g_hook_uid;
    p->plan_runs();
    *out = p.release();
    TF_API_END
}

// (the solver is not touched: a handle may outlive it; detach first -- tf_hook_attach(hook, 0, 0))
void tf_hook_destroy(tf_hook* p) { delete p; }

int tf_hook_set_x(tf_hook* p, const double* x) {
    TF_API_BEGIN
    require(p && x, "null argument");
    p->set_x(x);
    TF_API_END
}

int tf_hook_set_consts(tf_hook* p, const double* before, const double* after, double t_before, double t_after) {
    TF_API_BEGIN
    require(p && ((before && after) || p->nhc == 0), "null argument");
    tf_solver* s = p->solver;
    require(s->mode == tf_solver::TF_EAGER, "tf_hook_set_consts: not inside a step");
    const size_t n = (size_t)p->nhc * s->nsys;
    std::vector<double> cb(before, before + (before ? n : 0)), ca(after, after + (after ? n : 0));
    // (the times are kept for the record only: whatever of t a statement reads is one of the constants, so
    // the sets alone say what an application writes)
    p->t_before = t_before;
    p->t_after = t_after;
    // (uploaded in stream order, behind the steps queued so far; an unchanged set is not uploaded again)
    if (!p->have_consts || cb != p->consts) {
        if (n) p->set_consts("tf_hook", before, p->nhc);
        p->consts = cb;
    }
    if (!p->have_consts || ca != p->consts_post) {
        if (n) {
            std::vector<double> t(n, 0.0);                  // [nsys][nconst] -> [nconst][nsys]
            for (int e = 0; e < s->nsys; ++e)
                for (int k = 0; k < p->nhc; ++k) t[(size_t)k * s->nsys + e] = after[(size_t)e * p->nhc + k];
            tfb::h2d(p->hc_post.p, t.data(), n * sizeof(double), s->stream);
        }
        p->consts_post = ca;
    }
    p->have_consts = true;
    p->publish();
    TF_API_END
}

int tf_hook_attach(tf_hook* p, int32_t on, int32_t idempotent) {
    TF_API_BEGIN
    require(p, "null hook");
    tf_solver* s = p->solver;
    if (!on) { p->detach(); return 0; }
    require(s->prog == nullptr || s->prog == p, "tf_hook_attach: another program is attached to this solver");
    if (s->prog == p && s->prog_idem == (idempotent != 0)) return 0;
    s->drop_graphs();
    s->slot_hook.clear();
    s->prog = p; s->prog_apply = &tf_hook::apply_thunk; s->prog_idem = idempotent != 0; s->prog_uid = p->uid;
    p->publish();
    TF_API_END
}

int tf_hook_apply(tf_hook* p, int32_t src, int32_t dst) {
    TF_API_BEGIN
    require(p, "null hook");
    tf_solver* s = p->solver;
    double* U = s->st(dst);
    if (src != dst) tfb::d2d(U, s->st(src), (size_t)s->vecn() * sizeof(double), s->stream);
    s->slot_written(dst);
    p->run(U, false);
    TF_API_END
}

}  // extern "C"
