// TEST-ONLY host harness of the device probes: the generated probe block (codegen.lower_probes)
// and csrc/tf_probe.h compiled with g++ -- the per-node bodies and the chunk walks run as they
// do on the GPU, the shuffle / LDS trees of tfk_probe_partial / tfk_probe_final are replayed in
// their order (64-lane xor tree, four wavefronts of 256-thread workgroups; one wavefront per probe in
// tfk_probe_final).  Built per probe set
// by tests/probe_host/build_probe_host.py on tests/observer_host; never part of libtriflow_hip.so.
#include "observer_host.h"
#include "tf_probe.h"

namespace {
// the 64 lanes of a wavefront after tf_probe_wave: every lane holds the same value, lane 0's is taken
TfProbeAcc wave_tree(int kind, std::vector<TfProbeAcc> r) {
    for (int off = 32; off > 0; off >>= 1) {
        std::vector<TfProbeAcc> n(64);
        for (int l = 0; l < 64; ++l) n[l] = tf_probe_combine(kind, r[l], r[l ^ off]);
        r.swap(n);
    }
    return r[0];
}
// a workgroup of 256 threads: four wave trees, then the waves in order
TfProbeAcc block_tree(int kind, const std::vector<TfProbeAcc>& t) {
    TfProbeAcc r{};
    for (int w = 0; w < 4; ++w) {
        const TfProbeAcc v = wave_tree(kind, std::vector<TfProbeAcc>(t.begin() + 64 * w, t.begin() + 64 * w + 64));
        r = w == 0 ? v : tf_probe_combine(kind, r, v);
    }
    return r;
}
}  // namespace

extern "C" {

int probe_host_nprobe() { return TF_NPROBE; }

// out[nsys][nprobe]: the finished values of one record; nodes[nprobe][nsys][N]: the per-node values
int probe_host_run(const TfLayout* Lp, const double* fields, const double* helpers, const double* parvec,
                   const double* parsca, const double* dx, const double* xcoord, const double* hc,
                   double* out, double* nodes) {
    const TfLayout& L = *Lp;
    const int nblk = (L.P + 255) / 256, nseg = (L.M + TF_PROBE_SEG - 1) / TF_PROBE_SEG, nb = nblk * nseg;
    std::vector<double> partial((size_t)L.nsys * TF_NPROBE * nb * 2), ends((size_t)L.nsys * TF_NPROBE * 2);
    TfProbeArgs a{};
    static_cast<TfNodeArgs&>(a) = host_node_args(Lp, fields, helpers, parvec, parsca, dx, xcoord, hc);
    a.partial = partial.data(); a.ends = ends.data(); a.nblk = nblk; a.nseg = nseg;
    for (int e = 0; e < L.nsys; ++e) {
        for (int sb = 0; sb < nb; ++sb) {                             // tfk_probe_partial
            const int sg = sb / nblk, b = sb - sg * nblk;
            std::vector<std::vector<TfProbeAcc>> th(TF_NPROBE, std::vector<TfProbeAcc>(256));
            for (int t = 0; t < 256; ++t) {
                const int p = b * 256 + t;
                TfProbeAcc acc[TF_NPROBE_A];
                if (p < L.P) tf_probe_walk<true>(a, e, p, sg, acc, nodes);
                else for (int k = 0; k < TF_NPROBE; ++k) acc[k] = tf_probe_identity(tf_probe_kind[k]);
                for (int k = 0; k < TF_NPROBE; ++k) th[k][t] = acc[k];
            }
            for (int k = 0; k < TF_NPROBE; ++k) {
                const TfProbeAcc r = block_tree(tf_probe_kind[k], th[k]);
                double* o = a.partial + (((int64_t)e * TF_NPROBE + k) * nb + sb) * 2;
                o[0] = r.v; o[1] = r.i;
            }
        }
        for (int k = 0; k < TF_NPROBE; ++k) {                         // tfk_probe_final
            const int kind = tf_probe_kind[k];
            const double* part = a.partial + ((int64_t)e * TF_NPROBE + k) * nb * 2;
            std::vector<TfProbeAcc> th(64);                           // one wavefront per probe
            for (int t = 0; t < 64; ++t) {
                TfProbeAcc r = tf_probe_identity(kind);
                for (int b = t; b < nb; b += 64) r = tf_probe_combine(kind, r, TfProbeAcc{part[2 * b], part[2 * b + 1]});
                th[t] = r;
            }
            const TfProbeAcc r = wave_tree(kind, th);
            double xnode = 0.0;
            if ((kind == TF_PROBE_ARGMAX || kind == TF_PROBE_ARGMIN) && r.i >= 0.0 && r.i < (double)L.N) {
                int p, i;
                tf_locate(L, (int)r.i, p, i);
                xnode = xcoord[tf_idx(L, e * L.P + p, i)];
            }
            const double* end = a.ends + ((int64_t)e * TF_NPROBE + k) * 2;
            const double f0 = kind == TF_PROBE_INTEGRAL ? end[0] : 0.0;
            const double fN1 = kind == TF_PROBE_INTEGRAL ? end[1] : 0.0;
            out[(size_t)e * TF_NPROBE + k] = tf_probe_finish(kind, r, L.N, L.periodic, dx[e], f0, fN1, xnode);
        }
    }
    return 0;
}

}  // extern "C"
