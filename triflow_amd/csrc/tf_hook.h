// Device hooks: a program of statements  fields[var][target] = expression  that writes a resident state --
// boundary values tied to other nodes or fields, a sponge layer, a positivity clip -- where the reference
// calls hook(t, fields, pars) on the host.
//
// A statement's right-hand side is an expression in the model's string language, lowered by
// codegen.lower_hooks to one case of tf_eval_hook (same emitter as tf_eval_F and the observers' bodies: a
// value is the bits the lambdified NumPy code computes).  The contract (include/triflow_hip.h,
// tf_hook_apply) is the Python function that executes the statements in the order given, each right-hand
// side evaluated completely before its assignment, each statement seeing the assignments before it:
//   point   fields[var][node] = value     names are the fields at `node`; at(name, k) reads node k
//   window  fields[var][start:stop:step] = values     names are the fields at the node being assigned
// Every right-hand side of a window statement is pointwise (no stencil, no at(): refused when the program
// is built), so executing a run of window statements in order at each node equals executing it in order
// over whole arrays, and the nodes are independent of each other.
//
// The generated hook block defines TF_NHOOK, TF_NHOOK_HC, TF_HOOK_USES_X, TF_HOOK_MAXAT, tf_eval_hook and
// the static tables of the statements (tf_hook_kind, tf_hook_var, tf_hook_a / _b / _c, tf_hook_nat,
// tf_hook_at0, tf_hook_at_field, tf_hook_at_node) before this header is read: it is the tail of a hook code
// object's translation unit and of no other.  tfk_hook_window and tfk_hook_points are not in the kernel
// table (tf_args.h): the runtime finds them by name.
//
// The walks of one thread are what the host harness of the test suite (tests/hook_host/) also compiles
// with g++; the kernels are at the end of the file.  No LDS, no atomics, nothing contracted
// (-ffp-contract=off): a node belongs to one thread.
#pragma once
#include "tf_node.h"

// The inputs of a statement's body at ONE node of system e: the centre column of the register window (a
// hook reads no neighbours; the other columns stay zero and are never read), the node's vector parameters
// and x.  Fields are read from a.out, the pointer they are written through.
template <int NHC, bool USES_X>
struct TfHookNode {
    const TfHookArgs& a;
    const int e;
    double par[TF_NPAR > 0 ? TF_NPAR : 1];
    double hc[NHC > 0 ? NHC : 1];
    double dx, xc;
    double w[TF_NVAR + TF_NH][2 * TF_MP + 1];

    TF_DEVICE_M TfHookNode(const TfHookArgs& a_, int e_) : a(a_), e(e_) {
#pragma unroll
        for (int k = 0; k < TF_NPAR; ++k) par[k] = tf_par_is_vec[k] ? 0.0 : a.parsca[k * a.L.nsys + e];
#pragma unroll
        for (int k = 0; k < NHC; ++k) hc[k] = a.hc[k * a.L.nsys + e];
        dx = a.dx[e];
        xc = 0.0;
#pragma unroll
        for (int f = 0; f < TF_NVAR + TF_NH; ++f)
#pragma unroll
            for (int o = 0; o < 2 * TF_MP + 1; ++o) w[f][o] = 0.0;
    }
    // everything of the node at element s of the planes
    TF_DEVICE_M void load(int64_t s) {
#pragma unroll
        for (int f = 0; f < TF_NVAR + TF_NH; ++f)
            w[f][TF_MP] = f >= TF_NVAR ? a.helpers[(int64_t)(f - TF_NVAR) * a.L.plane + s]
                                       : a.out[(int64_t)f * a.L.plane + s];
#pragma unroll
        for (int k = 0; k < TF_NPAR; ++k)
            if (tf_par_is_vec[k]) par[k] = a.parvec[(int64_t)k * a.L.plane + s];
        xc = USES_X ? a.xcoord[s] : 0.0;
    }
};

// natural node g is one of the nodes window statement k assigns
TF_DEVICE bool tf_hook_assigns(int k, int g) {
    const int start = tf_hook_a[k], stop = tf_hook_b[k], step = tf_hook_c[k];
    return tf_hook_kind[k] == TF_HOOK_WINDOW && step >= 1 && g >= start && g < stop && (g - start) % step == 0;
}

// One thread, segment sg (TF_PROBE_SEG rows) of chunk p of system e, the window statements a.first ...
// a.first + a.count - 1: a row some statement assigns is loaded once (the centre values of all fields),
// the statements run on it in order, each masked by its own window, and the variables that were assigned
// are stored.  A row no statement assigns costs nothing.
TF_DEVICE void tf_hook_window_walk(const TfHookArgs& a, int e, int p, int sg) {
    const TfLayout& L = a.L;
    if (p < 0 || p >= L.P || sg < 0) return;
    const int len = tf_len(L, p);
    const int gstart = tf_start(L, p);
    const int i0 = sg * TF_PROBE_SEG;
    if (i0 >= len) return;
    const int kend = a.first + a.count < TF_NHOOK ? a.first + a.count : TF_NHOOK;
    const int kbeg = a.first > 0 ? a.first : 0;
    TfHookNode<TF_NHOOK_HC, TF_HOOK_USES_X> W(a, e);
    double noat[TF_HOOK_MAXAT];
#pragma unroll
    for (int j = 0; j < TF_HOOK_MAXAT; ++j) noat[j] = 0.0;
#pragma unroll
    for (int j = 0; j < TF_PROBE_SEG; ++j) {
        const int i = i0 + j;
        if (i >= len) break;
        const int g = gstart + i;
        bool any = false;
        for (int k = kbeg; k < kend; ++k) any = any || tf_hook_assigns(k, g);
        if (!any) continue;
        const int64_t s = tf_idx(L, e * L.P + p, i);
        W.load(s);
        unsigned dirty = 0u;
        for (int k = kbeg; k < kend; ++k) {
            if (!tf_hook_assigns(k, g)) continue;
            const double v = tf_eval_hook(k, W.w, W.par, W.hc, W.dx, W.xc, noat);
            const int var = tf_hook_var[k];
#pragma unroll
            for (int f = 0; f < TF_NVAR; ++f)
                if (f == var) { W.w[f][TF_MP] = v; dirty |= 1u << f; }
        }
#pragma unroll
        for (int f = 0; f < TF_NVAR; ++f)
            if ((dirty >> f) & 1u) a.out[(int64_t)f * L.plane + s] = W.w[f][TF_MP];
    }
}

// field f (dependent variables, then help functions) of system e at natural node g; 0.0 for what the
// tables should never name
TF_DEVICE double tf_hook_read(const TfHookArgs& a, int e, int f, int g) {
    const TfLayout& L = a.L;
    if (g < 0 || g >= L.N || f < 0 || f >= TF_NVAR + TF_NH) return 0.0;
    int p, i;
    tf_locate(L, g, p, i);
    const int64_t s = tf_idx(L, e * L.P + p, i);
    return f >= TF_NVAR ? a.helpers[(int64_t)(f - TF_NVAR) * L.plane + s] : a.out[(int64_t)f * L.plane + s];
}

// One thread, system e, the point statements a.first ... a.first + a.count - 1 in order: the at() reads
// of the statement are gathered, then the fields, the vector parameters and x of the target node, one
// value is evaluated and stored.  The next statement reads what this one wrote.
TF_DEVICE void tf_hook_points_walk(const TfHookArgs& a, int e) {
    const TfLayout& L = a.L;
    const int kend = a.first + a.count < TF_NHOOK ? a.first + a.count : TF_NHOOK;
    const int kbeg = a.first > 0 ? a.first : 0;
    TfHookNode<TF_NHOOK_HC, TF_HOOK_USES_X> W(a, e);
    for (int k = kbeg; k < kend; ++k) {
        const int g = tf_hook_a[k], var = tf_hook_var[k];
        if (tf_hook_kind[k] != TF_HOOK_POINT || g < 0 || g >= L.N || var < 0 || var >= TF_NVAR) continue;
        double at[TF_HOOK_MAXAT];
        const int nat = tf_hook_nat[k], at0 = tf_hook_at0[k];
#pragma unroll
        for (int j = 0; j < TF_HOOK_MAXAT; ++j)
            at[j] = j < nat ? tf_hook_read(a, e, tf_hook_at_field[at0 + j], tf_hook_at_node[at0 + j]) : 0.0;
        int p, i;
        tf_locate(L, g, p, i);
        const int64_t s = tf_idx(L, e * L.P + p, i);
        W.load(s);
        a.out[(int64_t)var * L.plane + s] = tf_eval_hook(k, W.w, W.par, W.hc, W.dx, W.xc, at);
    }
}

#if defined(__HIPCC__)
// grid (nsys * nblk, segments), 256 threads, one launch per run of window statements: the lanes of a
// wavefront sit over neighbouring chunks, so every load and store of a wavefront is 512 contiguous bytes.
// The grid covers the chunks a.p0 ... a.p1 - 1 and the segments from a.sg0 on: what the union of the run's
// windows touches (tf_rt_hook.cpp).
extern "C" __global__ void __launch_bounds__(256) tfk_hook_window(TfHookArgs a) {
    const int e = blockIdx.x / a.nblk, blk = blockIdx.x - e * a.nblk;
    const int p = a.p0 + blk * 256 + threadIdx.x;
    if (e < a.L.nsys && p < a.p1) tf_hook_window_walk(a, e, p, a.sg0 + (int)blockIdx.y);
}
// grid (ceil(nsys / 64)), 64 threads, one launch per run of point statements: one thread per system.
extern "C" __global__ void __launch_bounds__(64) tfk_hook_points(TfHookArgs a) {
    const int e = blockIdx.x * 64 + threadIdx.x;
    if (e < a.L.nsys) tf_hook_points_walk(a, e);
}
#endif
