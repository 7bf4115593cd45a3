// TEST-ONLY host harness of the device hooks: the generated hook block (codegen.lower_hooks) and
// csrc/tf_hook.h compiled with g++ -- the per-statement bodies and the walks of one thread run as they do on
// the GPU, one call per thread of a launch, a launch per run of statements, on the planes of one state in
// place.  A window run walks every chunk and every segment (the kernels' grid is the part of that the
// run's windows touch: tf_rt_hook.cpp; threads outside it find nothing to assign).  Built per program by
// tests/hook_host/build_hook_host.py; never part of libtriflow_hip.so.
#include "observer_host.h"
#include "tf_hook.h"

extern "C" {

int hook_host_nhook() { return TF_NHOOK; }
int hook_host_nconst() { return TF_NHOOK_HC; }

// runs[nruns][3]: kind, first, count; the state `fields` ([nvar] planes) is assigned in place
int hook_host_apply(const TfLayout* Lp, double* fields, const double* helpers, const double* parvec,
                    const double* parsca, const double* dx, const double* xcoord, const double* hc,
                    int nruns, const int* runs) {
    const TfLayout& L = *Lp;
    const int nseg = (L.M + TF_PROBE_SEG - 1) / TF_PROBE_SEG;
    TfHookArgs a{};
    static_cast<TfNodeArgs&>(a) = host_node_args(Lp, fields, helpers, parvec, parsca, dx, xcoord, hc);
    a.out = fields;
    for (int r = 0; r < nruns; ++r) {
        a.first = runs[3 * r + 1];
        a.count = runs[3 * r + 2];
        if (a.first < 0 || a.count < 1 || a.first + a.count > TF_NHOOK) return 1;
        for (int e = 0; e < L.nsys; ++e) {
            if (runs[3 * r] == TF_HOOK_POINT) { tf_hook_points_walk(a, e); continue; }
            a.p0 = 0; a.p1 = L.P; a.sg0 = 0; a.nblk = (L.P + 255) / 256;
            for (int sg = 0; sg < nseg; ++sg)
                for (int p = 0; p < L.P; ++p) tf_hook_window_walk(a, e, p, sg);
        }
    }
    return 0;
}

}  // extern "C"
