// TEST-ONLY host harness of the device spectra: the generated spectrum block (codegen.lower_spectra) and
// csrc/tf_spectrum.h compiled with g++ -- the per-node bodies, the twiddle function and the walk of one
// thread run as they do on the GPU, one call per thread of tfk_spectrum_partial's grid.  The per-thread
// (re, im) pairs are reduced in the kernels' fixed order: per workgroup of 256 threads the 64-lane xor
// tree of each of its four wavefronts (off = 32, 16, ... 1; every lane adds its partner), then the four
// wavefronts in order; per system and mode (tfk_spectrum_final) lane l adds the partials l, l + 64, ...
// in order, then the xor tree over the 64 lanes.  Built per spectrum set by
// tests/spectrum_host/build_spectrum_host.py; never part of libtriflow_hip.so.
#include "observer_host.h"
#include "tf_spectrum.h"

namespace {
double wave_tree(std::vector<double> r) {
    for (int off = 32; off > 0; off >>= 1) {
        std::vector<double> n(64);
        for (int l = 0; l < 64; ++l) n[l] = r[l] + r[l ^ off];
        r.swap(n);
    }
    return r[0];
}
double block_tree(const std::vector<double>& t) {
    double r = 0.0;
    for (int w = 0; w < 4; ++w) {
        const double v = wave_tree(std::vector<double>(t.begin() + 64 * w, t.begin() + 64 * w + 64));
        r = w == 0 ? v : r + v;
    }
    return r;
}
}  // namespace

extern "C" {

int spectrum_host_nspec() { return TF_NSPEC; }
int spectrum_host_max_modes() { return TF_SPEC_MAX_MODES; }

// exp(-2 pi i r / N) as the kernels compute it
void spectrum_host_twiddle(int64_t r, int64_t N, double* out) { tf_spec_twiddle(r, N, out, out + 1); }

// out[nsys][nmodes][2]: one row of expression `which` at the modes `modes`
int spectrum_host_run(const TfLayout* Lp, const double* fields, const double* helpers, const double* parvec,
                      const double* parsca, const double* dx, const double* xcoord, const double* hc,
                      int which, int nmodes, const int* modes, double* out) {
    const TfLayout& L = *Lp;
    const int nblk = (L.P + 255) / 256, nseg = (L.M + TF_PROBE_SEG - 1) / TF_PROBE_SEG, nb = nblk * nseg;
    if (nmodes < 1 || nmodes > TF_SPEC_MAX_MODES) return 1;
    TfSpectrumArgs a{};
    static_cast<TfNodeArgs&>(a) = host_node_args(Lp, fields, helpers, parvec, parsca, dx, xcoord, hc);
    a.which = which; a.nmodes = nmodes; a.nblk = nblk; a.nseg = nseg; a.modes = modes;
    std::vector<double> step((size_t)TF_PROBE_SEG * nmodes * 2);       // the table of a workgroup
    for (int j = 0; j < TF_PROBE_SEG; ++j)
        for (int k = 0; k < nmodes; ++k) tf_spec_step(modes[k], j, L.N, &step[((size_t)j * nmodes + k) * 2]);
    std::vector<double> partial((size_t)L.nsys * nmodes * nb * 2);
    for (int e = 0; e < L.nsys; ++e) {
        for (int sb = 0; sb < nb; ++sb) {                              // tfk_spectrum_partial
            const int sg = sb / nblk, b = sb - sg * nblk;
            std::vector<std::vector<double>> re(nmodes, std::vector<double>(256, 0.0)), im = re;
            for (int t = 0; t < 256; ++t) {
                const int p = b * 256 + t;
                double v[TF_PROBE_SEG];
                int n = 0, g0 = 0;
                if (p < L.P) n = tf_spectrum_values(a, e, p, sg, v, &g0);
                const double poison = tf_spectrum_poison(n, v);
                for (int k = 0; k < nmodes && n > 0; ++k)
                    tf_spectrum_mode(modes[k], g0, L.N, n, v, poison, &step[(size_t)k * 2], 2 * nmodes, &re[k][t], &im[k][t]);
            }
            for (int k = 0; k < nmodes; ++k) {
                double* o = &partial[(((size_t)e * nmodes + k) * nb + sb) * 2];
                o[0] = block_tree(re[k]);
                o[1] = block_tree(im[k]);
            }
        }
        for (int k = 0; k < nmodes; ++k) {                             // tfk_spectrum_final
            const double* part = &partial[((size_t)e * nmodes + k) * nb * 2];
            std::vector<double> re(64, 0.0), im(64, 0.0);
            for (int t = 0; t < 64; ++t)
                for (int b = t; b < nb; b += 64) { re[t] = re[t] + part[2 * b]; im[t] = im[t] + part[2 * b + 1]; }
            out[((size_t)e * nmodes + k) * 2] = wave_tree(re);
            out[((size_t)e * nmodes + k) * 2 + 1] = wave_tree(im);
        }
    }
    return 0;
}

}  // extern "C"
