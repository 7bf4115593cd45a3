// TEST-ONLY head of the host harnesses of the device observers (tests/probe_host, tests/record_host): the
// device qualifiers as g++ reads them, the generated translation unit of the model and the observer's block
// (TF_OBSERVER_HOST_HEADER, written by tests/observer_host/common.py) and the kernels' helpers.  The
// harness includes its observer's header (csrc/tf_probe.h, csrc/tf_record.h) after this one.
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

#define TF_DEVICE static inline
#define TF_DEVICE_M inline
#include "tf_args.h"
#include "tf_math.h"
using std::sqrt; using std::exp; using std::log; using std::sin; using std::cos; using std::tan;
using std::tanh; using std::sinh; using std::cosh; using std::pow; using std::atan; using std::asin;
using std::acos; using std::log10; using std::log2; using std::cbrt; using std::expm1; using std::log1p;
using std::floor; using std::ceil;
#include TF_OBSERVER_HOST_HEADER
#include "tf_kernels.h"

// the inputs of the node core, as common.system_planes lays them out
static inline TfNodeArgs host_node_args(const TfLayout* L, const double* fields, const double* helpers,
                                        const double* parvec, const double* parsca, const double* dx,
                                        const double* xcoord, const double* hc) {
    return TfNodeArgs{*L, fields, helpers, parvec, parsca, dx, xcoord, hc};
}
