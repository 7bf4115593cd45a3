// TEST-ONLY host harness of the index mapping of the wide memory phases of tfk_cr_factor_v4
// (csrc/tf_cr_io.h) compiled with g++: for every block size 3 ... 8, chunk length 1 ... 16 and workgroup of
// 256 and 512 threads, the threads of a workgroup are run one after the other through the mapping as the
// kernel uses it, and what they touch is held against the loops of the kernel's TF_CR_WIDE_IO=0 form, which
// are copied below with their own index arithmetic:
//   load    every LDS slot the loops load is loaded exactly once and from the same record entries (one
//           entry, or the two parts of a diagonal entry, which one thread holds and adds); every slot the
//           loops set to zero is set to zero exactly once; nothing else is written; every 16-byte request
//           is aligned and lies inside the chunk;
//   share   the same entries of the next level's records and right-hand sides are stored, once each, from
//           the same slots;
//   record  entry e of [Dinv | E | F] is read from the slot its lane staged it in, and no two lanes stage
//           to one slot.
// Prints one line per failure and returns their number.  Built and run by tests/cr_io_host/build_cr_io_host.py.
#include <cstdio>
#include <map>
#include <tuple>
#include <vector>

#include "tf_cr_io.h"

namespace {
constexpr int MAXLEN = 16, NPOS = MAXLEN + 1, NT_MIN = 256;

struct Slot {
    int loads = 0, zeros = 0, src1 = -1, src2 = -1;
    bool operator==(const Slot& o) const { return loads == o.loads && zeros == o.zeros && src1 == o.src1 && src2 == o.src2; }
};

int fails = 0;
#define FAIL(...) do { if (++fails <= 40) { std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

template <int BB>
void check_load(int len, int NT) {
    typedef TfCrWide<BB> Io;
    constexpr int B2 = BB * BB, REC = 4 * B2, RS = Io::RS, PS = Io::PS;
    std::vector<Slot> want(NPOS * PS), got(NPOS * PS);
    // ---- the loops of the TF_CR_WIDE_IO=0 form
    const int n3 = len * 3 * B2;
    for (int tid = 0; tid < NT; ++tid) {
        for (int i = tid; i < (len + 1) * BB * (RS - 3 * BB); i += NT) {
            const int pr = i / (RS - 3 * BB), o = i - pr * (RS - 3 * BB);
            want[(pr / BB) * PS + (pr % BB) * RS + 3 * BB + o].zeros++;
        }
        if (tid < 3 * B2) {
            const int blk = tid / B2, rc = tid - blk * B2, r = rc / BB, cc = rc - r * BB;
            want[0 * PS + r * RS + blk * BB + cc].zeros++;
        }
        constexpr int NIT = (MAXLEN * 3 * B2 + NT_MIN - 1) / NT_MIN;
        for (int it = 0; it < NIT; ++it) {
            const int i = it * NT + tid;
            const int nd = i / (3 * B2), rem = i - nd * 3 * B2, blk = rem / B2, rc = rem - blk * B2;
            const int r = rc / BB, cc = rc - r * BB;
            if (i < n3) {
                Slot& s = want[(nd + 1) * PS + r * RS + blk * BB + cc];
                s.loads++;
                s.src1 = nd * REC + blk * B2 + rc;
                s.src2 = blk == 1 ? nd * REC + 3 * B2 + rc : -1;
            }
        }
    }
    // ---- the wide form
    constexpr int NITW = (MAXLEN + NT_MIN / B2 - 1) / (NT_MIN / B2);
    const int npi = Io::nodes_per_pass(NT);
    for (int tid = 0; tid < NT; ++tid) {
        int ndl, q;
        bool act;
        Io::thread(tid, NT, ndl, q, act);
        for (int i = tid; i < PS; i += NT) got[i].zeros++;
        for (int it = 0; it < NITW; ++it) {
            const int nd = ndl + it * npi, ndc = nd < len ? nd : len - 1;
            const int a0 = ndc * REC + 2 * q, b0 = a0 + 2 * B2;        // the two 16-byte requests, in doubles
            if (a0 % 2 || a0 < 0 || b0 + 1 >= len * REC) FAIL("b %d len %d NT %d tid %d: request out of the chunk", BB, len, NT, tid);
            if (!(act && nd < len)) continue;
            for (int h = 0; h < 2; ++h) {
                int slot;
                bool dia;
                Io::pair(q, h, slot, dia);
                Slot& s = got[(nd + 1) * PS + slot];
                s.loads++; s.src1 = a0 + h; s.src2 = dia ? b0 + h : -1;
                if (!dia) {
                    Slot& u = got[(nd + 1) * PS + slot + 2 * BB];
                    u.loads++; u.src1 = b0 + h; u.src2 = -1;
                }
            }
            for (int j = 0; j < Io::NZ; ++j) {
                const int z = Io::zero_slot(q, j);
                if (z >= 0) got[(nd + 1) * PS + z].zeros++;
            }
        }
    }
    for (int i = 0; i < NPOS * PS; ++i) {
        if (want[i].loads + want[i].zeros > 1) FAIL("b %d len %d NT %d: the reference loops write slot %d twice", BB, len, NT, i);
        if (!(want[i] == got[i]))
            FAIL("b %d len %d NT %d slot %d: loads %d/%d zeros %d/%d sources (%d, %d)/(%d, %d)", BB, len, NT, i, got[i].loads,
                 want[i].loads, got[i].zeros, want[i].zeros, got[i].src1, got[i].src2, want[i].src1, want[i].src2);
    }
}

// key: (0 record / 1 right-hand side, side, offset in the record or the rhs) -> (position 0 / last, slot, second slot)
typedef std::map<std::tuple<int, int, int>, std::tuple<int, int, int>> Share;

template <int BB>
void check_share(int NT) {
    typedef TfCrWide<BB> Io;
    constexpr int B2 = BB * BB, RS = Io::RS, NO = 2 * BB + 1;
    constexpr int oL = Io::oL, oDL = Io::oDL, oU = Io::oU, oYL = Io::oYL, oDR = Io::oDR, oYR = Io::oYR;
    Share want, got;
    int twice = 0;
    auto put = [&](Share& m, int kind, int side, int off, int slot, int slot2) {
        if (!m.emplace(std::make_tuple(kind, side, off), std::make_tuple(side == 0 ? 1 : 0, slot, slot2)).second) ++twice;
    };
    for (int tid = 0; tid < NT; ++tid)
        for (int i = tid; i < 2 * BB * NO; i += NT) {
            const int side = i / (BB * NO), rem = i - side * BB * NO, r = rem / NO, o = rem - r * NO;
            if (o < BB) put(want, 0, side, (side == 0 ? 0 : 2) * B2 + r * BB + o, r * RS + (side == 0 ? oL : oU) + o, -1);
            else if (o < 2 * BB) put(want, 0, side, (side == 0 ? 1 : 3) * B2 + r * BB + o - BB, r * RS + oDL + o - BB, r * RS + oDR + o - BB);
            else put(want, 1, side, (side == 0 ? 0 : BB) + r, r * RS + oYL, r * RS + oYR);
        }
    for (int tid = 0; tid < NT; ++tid) {
        int side, q, r;
        bool act;
        Io::share_thread(tid, side, q, act);
        if (act)
            for (int h = 0; h < 2; ++h) {
                int slot;
                bool dia;
                Io::pair(q, h, slot, dia);
                // the kernel: first slot = slot (+ 2 BB for the U block of side 1), second = first + oDR - oDL
                const int first = dia ? slot : slot + side * 2 * BB;
                put(got, 0, side, side * 2 * B2 + 2 * q + h, first, dia ? first + oDR - oDL : -1);
            }
        Io::share_rhs_thread(tid, side, r, act);
        if (act) put(got, 1, side, (side == 0 ? 0 : BB) + r, r * RS + oYL, r * RS + oYR);
    }
    if (twice) FAIL("b %d NT %d: %d entries of the share stored twice", BB, NT, twice);
    if (want != got) FAIL("b %d NT %d: the share differs (%zu / %zu entries)", BB, NT, got.size(), want.size());
    if (2 * Io::SH + 2 * BB > NT_MIN) FAIL("b %d: the share needs more threads than the workgroup has", BB);
}

template <int BB>
void check_record() {
    typedef TfCrWide<BB> Io;
    constexpr int B2 = BB * BB, RS = Io::RS, NC = 4 * BB + 1;
    std::vector<int> staged(3 * B2, -1), owner(Io::PS, 0);
    for (int c = 0; c < NC; ++c) {
        // the lane classes of the kernel: columns of [L | D | U | y | I]
        const bool cL = c < BB, cD = c >= BB && c < 2 * BB, cU = c >= 2 * BB && c < 3 * BB, cY = c == 3 * BB, cI = c > 3 * BB;
        if (cD) continue;
        const int idc = c - 3 * BB - 1;
        const int soff = cI ? Io::oDR + idc : (cL ? Io::oL + c : (cU ? Io::oU + c - 2 * BB : Io::oYL));
        for (int i = 0; i < BB; ++i) {
            if (owner[i * RS + soff]++) FAIL("b %d: two lanes stage to slot %d", BB, i * RS + soff);
            if (cY) continue;
            const int e = (cI ? idc : (cL ? B2 + c : 2 * B2 + c - 2 * BB)) + i * BB;     // goff / 8 + i * BB
            if (staged[e] != -1) FAIL("b %d: record entry %d staged twice", BB, e);
            staged[e] = i * RS + soff;
        }
    }
    for (int e = 0; e < 3 * B2; ++e)
        if (staged[e] != Io::record_slot(e)) FAIL("b %d: record entry %d staged in slot %d, read from %d", BB, e, staged[e], Io::record_slot(e));
}

template <int BB>
void check_all() {
    for (int NT = 256; NT <= 512; NT += 256) {
        for (int len = 1; len <= MAXLEN; ++len) check_load<BB>(len, NT);
        check_share<BB>(NT);
    }
    check_record<BB>();
}
}  // namespace

int main() {
    check_all<3>(); check_all<4>(); check_all<5>(); check_all<6>(); check_all<7>(); check_all<8>();
    std::printf("%d failures\n", fails);
    return fails ? 1 : 0;
}
