// TEST-ONLY host harness of the device recorders: the generated record block (codegen.lower_records)
// and csrc/tf_record.h compiled with g++ -- the per-node bodies and the walks run as they do on the
// GPU, the parts of a bin meet in the order tfk_record combines them in (tf_record_finish over the
// parts of a workgroup's LDS).  Built per recorder set by tests/record_host/build_record_host.py;
// never part of libtriflow_hip.so.
#include "observer_host.h"
#include "tf_record.h"

extern "C" {

int record_host_nrec() { return TF_NREC; }

// out[nsys][ncols]: one row of recorder `which`; geometry as tf_record_create lays it out
int record_host_run(const TfLayout* Lp, const double* fields, const double* helpers, const double* parvec,
                    const double* parsca, const double* dx, const double* xcoord, const double* hc,
                    int which, int pool, int start, int stop, int step, double* out) {
    TfRecordArgs a{};
    static_cast<TfNodeArgs&>(a) = host_node_args(Lp, fields, helpers, parvec, parsca, dx, xcoord, hc);
    a.which = which; a.pool = pool; a.start = start; a.stop = stop; a.step = step;
    a.ncols = (stop - start + step - 1) / step;
    a.split = 1;
    if (pool != TF_REC_SAMPLE)
        while (a.split < TF_REC_BLOCK && a.split * 8 < step) a.split *= 2;
    a.part = pool == TF_REC_SAMPLE ? 1 : (step + a.split - 1) / a.split;
    std::vector<double> parts(a.split);
    for (int e = 0; e < a.L.nsys; ++e)
        for (int j = 0; j < a.ncols; ++j) {
            for (int s = 0; s < a.split; ++s)
                parts[s] = s * a.part < tf_rec_count(a, j) ? tf_record_part(a, e, j, s) : 0.0;
            out[(size_t)e * a.ncols + j] = tf_record_finish(a, j, parts.data());
        }
    return 0;
}

}  // extern "C"
