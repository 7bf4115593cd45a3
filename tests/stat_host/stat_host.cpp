// TEST-ONLY host harness of the device statistics: the generated statistic block
// (codegen.lower_statistics) and csrc/tf_stat.h compiled with g++ -- the per-node bodies, the walk and the
// fold run as they do on the GPU, one call per thread of tfk_stat's grid.  Built per statistic set by
// tests/stat_host/build_stat_host.py; never part of libtriflow_hip.so.
#include "observer_host.h"
#include "tf_stat.h"

extern "C" {

int stat_host_nstat() { return TF_NSTAT; }
int stat_host_planes(int kind) { return tf_stat_planes(kind); }

// sample k, taken at t, of expression `which` into acc[tf_stat_planes(kind)] planes
int stat_host_update(const TfLayout* Lp, const double* fields, const double* helpers, const double* parvec,
                     const double* parsca, const double* dx, const double* xcoord, const double* hc,
                     int which, int kind, double k, double t, double* acc) {
    TfStatArgs a{};
    static_cast<TfNodeArgs&>(a) = host_node_args(Lp, fields, helpers, parvec, parsca, dx, xcoord, hc);
    a.which = which; a.kind = kind; a.k = k; a.t = t; a.acc = acc;
    a.nblk = (a.L.P + 255) / 256;
    a.nseg = (a.L.M + TF_PROBE_SEG - 1) / TF_PROBE_SEG;
    for (int e = 0; e < a.L.nsys; ++e)
        for (int blk = 0; blk < a.nblk; ++blk)
            for (int sg = 0; sg < a.nseg; ++sg)
                for (int tid = 0; tid < 256; ++tid) {
                    const int p = blk * 256 + tid;
                    if (p < a.L.P) tf_stat_walk(a, e, p, sg);
                }
    return 0;
}

}  // extern "C"
