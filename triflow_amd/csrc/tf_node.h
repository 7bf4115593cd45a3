// The node core of the device observers (probes: tf_probe.h, recorders: tf_record.h): a model expression
// evaluated at the nodes of a resident state slot.  The generated per-node bodies (tf_eval_probe,
// tf_eval_record: same emitter as tf_eval_F) read a register window of the fields around the node, the
// parameters, the host constants of the expressions, dx and x; TfNodeWindow loads and slides that window
// for one thread, whatever the thread does with the values.  An observer supplies its walk (which nodes,
// in which order, folded how), its kernels and its ring; TfNodeArgs (tf_args.h) leads its arguments.
//
// Compiled by hipcc into every observer's code object, and into none of the solver's, and by g++ into the
// host harnesses of the test suite (tests/probe_host, tests/record_host ...).
#pragma once
#include "tf_layout.h"          // tf_idx, tf_nbr

// A value and the natural node index it was met at (a double: exact for any node count a plane can hold).
struct TfNodeAcc { double v, i; };

// b after a, for a maximum (up) or a minimum as numpy has it: NaN wins.  The result does not depend on
// the order of the operands (among NaNs and among equal values the pairs differ in the index only, which
// a maximum / minimum does not report), so any tree gives numpy's answer.
TF_DEVICE TfNodeAcc tf_node_extremum(bool up, TfNodeAcc a, TfNodeAcc b) {
    const bool anan = a.v != a.v, bnan = b.v != b.v;
    if (anan) return a;
    if (bnan) return b;
    const bool take = up ? b.v > a.v : b.v < a.v;
    return take ? b : a;
}

// The inputs of the per-node body of system e for one thread.  NHC: host constants of the expressions,
// USES_X: an expression reads x (else no x plane is touched).  The window slides along the rows of a
// chunk as in the F sweep (tfk_sweep_body): prime(p, len, i) then advance(p, len, i), advance(p, len,
// i + 1) ...; rows outside 0 ... len - 1 of chunk p are ghosts through tf_nbr, wrapped or clamped at the
// ends of the system.  A walk that leaves its chunk goes on at row 0 of the next one with the window it holds.
template <int NHC, bool USES_X>
struct TfNodeWindow {
    const TfNodeArgs& a;
    const int e;
    double par[TF_NPAR > 0 ? TF_NPAR : 1];
    double hc[NHC > 0 ? NHC : 1];
    double dx, xc;
    double w[TF_NVAR + TF_NH][2 * TF_MP + 1];

    TF_DEVICE_M TfNodeWindow(const TfNodeArgs& a_, int e_) : a(a_), e(e_) {
#pragma unroll
        for (int k = 0; k < TF_NPAR; ++k) par[k] = tf_par_is_vec[k] ? 0.0 : a.parsca[k * a.L.nsys + e];
#pragma unroll
        for (int k = 0; k < NHC; ++k) hc[k] = a.hc[k * a.L.nsys + e];
        dx = a.dx[e];
    }
    // field f (dependent variables, then help functions) at row ii of chunk p, of len rows
    TF_DEVICE_M double ld(int p, int len, int f, int ii) const {
        const TfLayout& L = a.L;
        const int64_t s = (ii >= 0 && ii < len) ? tf_idx(L, e * L.P + p, ii) : tf_nbr(L, e, p, len, 0, ii);
        return f >= TF_NVAR ? a.helpers[(int64_t)(f - TF_NVAR) * L.plane + s]
                            : a.fields[(int64_t)f * L.plane + s];
    }
    // the window one node short of row i: the advance to (p, i) completes it
    TF_DEVICE_M void prime(int p, int len, int i) {
#pragma unroll
        for (int f = 0; f < TF_NVAR + TF_NH; ++f)
#pragma unroll
            for (int o = 1; o < 2 * TF_MP + 1; ++o) w[f][o] = ld(p, len, f, i + o - 1 - TF_MP);
    }
    // one node on, to row i of chunk p: the new right column, the node's vector parameters and x
    TF_DEVICE_M void advance(int p, int len, int i) {
#pragma unroll
        for (int f = 0; f < TF_NVAR + TF_NH; ++f) {
#pragma unroll
            for (int o = 0; o < 2 * TF_MP; ++o) w[f][o] = w[f][o + 1];
            w[f][2 * TF_MP] = ld(p, len, f, i + TF_MP);
        }
        const int64_t s = tf_idx(a.L, e * a.L.P + p, i);
#pragma unroll
        for (int k = 0; k < TF_NPAR; ++k)
            if (tf_par_is_vec[k]) par[k] = a.parvec[(int64_t)k * a.L.plane + s];
        xc = USES_X ? a.xcoord[s] : 0.0;
    }
};
