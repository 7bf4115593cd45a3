// TEST-ONLY: host harness of RowRing and HalfRing (csrc/tf_solver.h), the rings of rows of the device
// observers (HalfRing: the recorders' two halves; the emulation's copies are synchronous).  Linked with tests/emu/tf_backend_emu.cpp, whose device memory is the host's (dev_alloc is
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

// ---- HalfRing: the same five entry points; capacity = both halves
void* half_host_create(int capacity, int row) {
    HalfRing* r = new HalfRing();
    r->half = capacity / 2;
    r->row = (size_t)row;
    int64_t bytes = 0;
    r->alloc(bytes);
    return r;
}

void half_host_destroy(void* p) { delete (HalfRing*)p; }

int half_host_push(void* p, double tag) {
    HalfRing& r = *(HalfRing*)p;
    const int at = r.begin_row(nullptr);
    if (at < 0 || at >= 2 * r.half) return -1;
    for (size_t j = 0; j < r.row; ++j) r.dev.p[(size_t)at * r.row + j] = tag + 0.25 * (double)j;
    r.end_row(nullptr, nullptr);
    return at;
}

int64_t half_host_fetch(void* p, double* out, int64_t max_rows) {
    int64_t n = -1;
    ((HalfRing*)p)->fetch(nullptr, nullptr, out, max_rows, &n);
    return n;
}

int64_t half_host_pending(void* p) { return ((const HalfRing*)p)->pending(); }

}  // extern "C"
