// Index mapping of the memory phases of tfk_cr_factor_v4 (tf_cr3_hip.h, TF_CR_WIDE_IO): which thread moves
// which 16 bytes of a chunk's node records, and where they go in LDS.  Plain integer arithmetic that also
// compiles on the host (tests/cr_io_host holds it against the loops it replaces).
//
// A node record [L | D | U | second part of D][b][b] is two halves of the same shape, [L | D] and [U | D2],
// 2 b^2 doubles = b^2 pairs of 16 bytes each (a record starts on a multiple of 32 b^2 bytes, a half on a
// multiple of 16 b^2: every pair is 16-byte aligned for every b).  Pair q of the first half and pair q of the
// second hold, element by element, either (an entry of L, the same entry of U) or (the two parts of one
// entry of D): one thread loads both pairs, and the sum of the two parts is one addition in that thread.
// For odd b the middle pair holds the last entry of L / U and the first of D / D2; the rule is per element.
//
// A thread keeps its pair q for the whole kernel and takes the nodes ndl, ndl + npi, ndl + 2 npi ... of the
// chunk (npi = NT / b^2 nodes per pass), so its LDS slots inside a chain position are worked out once.
#pragma once

#if defined(__HIPCC__)
#define TF_CRIO_FN __host__ __device__ __forceinline__
#else
#define TF_CRIO_FN inline
#endif

template <int BB> struct TfCrWide {
    static constexpr int B2 = BB * BB, REC = 4 * B2;
    // the block row of a chain position in LDS (TfCr3<BB>): [L | DL | U | yL | DR | yR | 0]
    static constexpr int oL = 0, oDL = BB, oU = 2 * BB, oYL = 3 * BB, oDR = 3 * BB + 1, oYR = 4 * BB + 1;
    static constexpr int RS = (4 * BB + 3) | 1, PS = BB * RS;
    // the slots of a block row that no record entry goes to (yL, DR, yR, the zero slot, the padding)
    static constexpr int ZW = RS - 3 * BB, NZS = BB * ZW, NZ = (NZS + B2 - 1) / B2;

    // nodes per pass of a workgroup of nt threads; thread tid -> (node of the first pass, pair)
    static TF_CRIO_FN int nodes_per_pass(int nt) { return nt / B2; }
    static TF_CRIO_FN void thread(int tid, int nt, int& ndl, int& q, bool& active) {
        ndl = tid / B2; q = tid - ndl * B2; active = ndl < nodes_per_pass(nt);
    }
    // element h (0, 1) of pair q of a half record: `dia` -- it is an entry of D (first half) / D2 (second half)
    // and the sum of the two goes to `slot`; else the first half's value (L) goes to `slot`, the second half's
    // (U) to `slot + 2 BB`.  `slot` is relative to the chain position's first row.
    static TF_CRIO_FN void pair(int q, int h, int& slot, bool& dia) {
        const int e = 2 * q + h;
        dia = e >= B2;
        const int rc = dia ? e - B2 : e, r = rc / BB, cc = rc - r * BB;
        slot = r * RS + (dia ? oDL : oL) + cc;
    }
    // the j-th (j < NZ) slot that the thread of pair q sets to zero in each of its positions, or -1
    static TF_CRIO_FN int zero_slot(int q, int j) {
        const int z = q + j * B2;
        if (z >= NZS) return -1;
        const int r = z / ZW;
        return r * RS + 3 * BB + (z - r * ZW);
    }
    // the share of the next level's rows: threads [0, B2) store the first half of a record from the rows of the
    // last position, threads [SH, SH + B2) the second half of another record from position 0, a pair each;
    // threads [2 SH, 2 SH + 2 BB) the two right-hand sides
    static constexpr int SH = (B2 + 63) & ~63;
    static TF_CRIO_FN void share_thread(int tid, int& side, int& q, bool& active) {
        side = tid >= SH ? 1 : 0; q = tid - side * SH; active = q >= 0 && q < B2;
    }
    static TF_CRIO_FN void share_rhs_thread(int tid, int& side, int& r, bool& active) {
        const int t = tid - 2 * SH;
        side = t >= BB ? 1 : 0; r = t - side * BB; active = t >= 0 && t < 2 * BB;
    }
    // record [Dinv | E | F][b][b] of an eliminated node, staged in its own (dead) rows: Dinv in the DR slots,
    // E in L, F in U.  Entry e of the record -> slot relative to the position's first row
    static TF_CRIO_FN int record_slot(int e) {
        const int blk = e / B2, rc = e - blk * B2, i = rc / BB, cc = rc - i * BB;
        return i * RS + (blk == 0 ? oDR : (blk == 1 ? oL : oU)) + cc;
    }
};
