// TEST-ONLY: host harness of RowRing (csrc/tf_solver.h), the ring of rows of the device spectra, extrema and
// histograms.  Linked with tests/emu/tf_backend_emu.cpp, whose device memory is the host's (dev_alloc is
// calloc, d2h is memcpy), so the ring's bookkeeping -- the part of those observers that no CPU test of the
// kernels reaches -- runs without a GPU.  The "kernel" is push: a host write of a recognisable row at the
// index the ring hands out.
#include "tf_solver.h"

extern "C" {

void* ring_host_create(int capacity, int row) {
    RowRing* r = new RowRing();
    r->capacity = capacity;
    r->row = (size_t)row;
    int64_t bytes = 0;
    r->alloc(bytes);
    return r;
}

void ring_host_destroy(void* p) { delete (RowRing*)p; }

// one record: row (tag, tag + 0.25, ...) at the index the ring hands out, which is returned (-1: the index
// is outside the ring, nothing was written)
int ring_host_push(void* p, double tag) {
    RowRing& r = *(RowRing*)p;
    const int at = r.next_row(nullptr);
    if (at < 0 || at >= r.capacity) return -1;
    for (size_t j = 0; j < r.row; ++j) r.ring.p[(size_t)at * r.row + j] = tag + 0.25 * (double)j;
    ++r.on_device;
    return at;
}

int64_t ring_host_fetch(void* p, double* out, int64_t max_rows) {
    int64_t n = -1;
    ((RowRing*)p)->fetch(nullptr, out, max_rows, &n);
    return n;
}

int64_t ring_host_pending(void* p) { return ((const RowRing*)p)->pending(); }

}  // extern "C"
