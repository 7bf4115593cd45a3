// Plain-data launch argument blocks shared by the host runtime (tf_solver.h, tf_rt_*.cpp)
// and the per-model kernels (tf_kernels.h).  Every kernel takes exactly one of
// these structs by value.
#pragma once
#include <stdint.h>

#define TF_MAX_FIELDS 16   // dependent variables + help functions
#define TF_MAX_PARS 16
#define TF_MAX_TERMS 8

// Partition-interleaved layout of one solver level.
//
// A system of N nodes is cut into P chunks of consecutive nodes; the first
// `rem` chunks own mbase+1 nodes, the others mbase.  Node i of chunk p of
// system e is stored at element  i * Ptot + (e * P + p)  of a plane, so that
// the 64 lanes of a wavefront, which work on 64 neighbouring chunks, always
// touch 512 contiguous bytes, whatever i is.  One thread then walks *along* a
// chunk with its stencil neighbourhood in registers.
struct TfLayout {
    int nsys;      // independent systems (ensemble members)
    int N;         // nodes per system
    int P;         // chunks per system
    int mbase;     // base chunk length
    int rem;       // chunks [0, rem) are one node longer
    int M;         // rows of a plane = mbase + (rem > 0)
    int Ptot;      // nsys * P = row stride of a plane
    int periodic;
    int64_t plane; // M * Ptot elements
};

struct TfSweepArgs {               // F / F+J stencil sweep, J @ v, A-row build
    TfLayout L;
    const double* fields;          // [nvar] planes: dependent variables
    const double* helpers;         // [nh] planes: help functions
    const double* parvec;          // [npar] planes (only those flagged vector are read)
    const double* parsca;          // [npar][nsys] scalar parameter values
    const double* dx;              // [nsys]
    const double* xcoord;          // 1 plane (only read when the model uses x)
    double* F;                     // [nvar] planes
    double* Jv;                    // [nnz] planes (raw values, reference pattern order)
    int with_j;
    // Rosenbrock stage state evaluated on the fly: fields + (((kc0*kx0) + kc1*kx1) + ...)
    int nterms;
    const double* kx[TF_MAX_TERMS];
    double kc[TF_MAX_TERMS];
    double fscale;                 // F is stored as fscale * F (dt * F: the first stage's right-hand side)
    // tfk_sweep_fj_theta: also the right-hand side of the theta scheme in the same pass,
    //   rhs = dt * (F - (theta * J) @ U) + U        (schemes.py:553-556)
    double* theta_rhs;
    double theta, theta_dt;
    // tfk_sweep_fj_bdf2: right-hand side of the linearly implicit BDF-2 step and the history
    // update in the same pass:  rhs = c0*(U - Uprev) + c1*F (two_step) or c1*F;  Uprev <- U
    // (bdf_prev_out NULL: the history is not copied -- the caller keeps U_n in a state slot of its
    // own, tf_step_bdf2_from)
    double* bdf_rhs;
    const double* bdf_prev;
    double* bdf_prev_out;
    double bdf_c0, bdf_c1;
    int bdf_two_step;
    // F+J sweeps, 1: the node-independent planes of Jv (tf_j_uniform) already hold the values of the
    // current scalar parameters and dx (an earlier sweep wrote them); this launch leaves them alone.
    // (In the padding behind bdf_two_step: no other argument moves.)
    int ju_valid;
    // tfk_sweep_f_stage_rhs: the right-hand side of Rosenbrock stage i in the pass that evaluates
    // its F:  rhs = cF*(fscale*F(U + sum_j kc_j k_j)) + cA*(J @ (sum_j gc_j k_j)), the operations of
    // tfk_sweep_f_stage followed by tfk_spmv's stage form, in their order (schemes.py:152-160).
    // F itself is not stored; Jv is read (the entries that are not node-independent).
    double* stage_rhs;
    double gc[TF_MAX_TERMS];
    double cF, cA;
};

struct TfSpmvArgs {                // y = scale * J @ v  (clamped/wrapped columns)
    TfLayout L;
    const double* parsca;          // scalar parameters / dx: the node-independent Jacobian entries
    const double* dx;              // are evaluated in the kernel, not read back (TfJUniform)
    const double* Jv;
    const double* v;               // [nvar] planes
    double* y;                     // [nvar] planes
    double scale;
    int absval;                    // 1: y = |scale J| @ |v|  (componentwise backward error)
    // Rosenbrock stage right-hand side in one pass: v = ((vc0*vx0) + vc1*vx1) + ...,
    // y = cF*addF + cA*(J @ v)        (schemes.py:156-160)
    int nterms;
    const double* vx[TF_MAX_TERMS];
    double vc[TF_MAX_TERMS];
    const double* addF;
    double cF, cA;
};

struct TfNormArgs {               // per-variable, per-system norm of (a - b): partial sums
    TfLayout L;
    const double* a;               // [nvar] planes
    const double* b;
    double* partial;               // [nvar*nsys][nblocks]
    int nblocks;
    int ord;                       // 2: sum of squares, 0: max |.|
    // non-NULL: the failure flag and the monitor's worst value ride along behind the partials
    // (partial[nvar*nsys*nblocks], [.. + 1]): one download, one host wait per trial
    const int* status;
    const double* mon;
};

struct TfBerrArgs {               // componentwise backward error of (I - cJ) x = b
    TfLayout L;
    const double* parsca;
    const double* dx;
    const double* Jv;
    const double* x;               // [nvar] planes
    const double* rhs;             // [nvar] planes
    double c;
    double* red;                   // max_i |b - Ax|_i / (|x| + |cJ||x| + |b|)_i
    // Sampled form (the monitor of the Theta / BDF-2 steps), one_node >= 0: a thread looks at ONE node of
    // its chunk, node one_node modulo the chunk's length (grid.y = 1); -1: every node of segment grid.y
    int one_node;
    int reserved_;
    // non-NULL: x holds a new state U+ = xbase + delta and the system is (I - cJ) delta = b, i.e.
    // (I - cJ) U+ = b + (I - cJ) xbase: the error is measured on that form (magnitudes |U+| + |xbase|) --
    // delta itself is not in memory when the back-substitution forms the new state, and U+ - xbase
    // carries the rounding of the sum
    const double* xbase;
};

// tfk_sweep_f_stage_rhs_mon: the stage pass and, as one more row of workgroups, the sampled backward-error
// probe of the solve before it (TfBerrArgs::one_node >= 0)
struct TfStageMonArgs { TfSweepArgs s; TfBerrArgs b; };

// tfk_sweep_f_erk_last / _n: the last stage of an explicit Runge-Kutta step (tf_step_erk) with the update
// and the error estimate in the same pass.  s: the stage sweep -- fields = U, fscale = dt, and the s.nterms
// earlier stage vectors k_j (ascending j) that any of the three sums below reads: s.kc[t] is a_{s-1,j} and
// may be 0.0, then k_j is no part of the stage state and is loaded at the centre node only.  The kernel
// holds k_last = dt * F(U + sum a k) of its nodes in registers and writes
//   out = U + (((b[0]*k_0) + b[1]*k_1) + ... + b_last*k_last)                 (TF_VEC_SUM's order)
//   red = max(red, max over its nodes of |((d[0]*k_0) + ...) + d_last*k_last|)   (with_d; TF_VEC_MAXABS, NaN wins)
// A term whose coefficient is exactly 0.0 is left out of its sum (b_last / d_last included).  Not in the
// kernel table: resolved by name (tfb::kernel_lookup), like the histogram kernels; the emulation never
// launches it.
struct TfErkTail {
    double* out;                   // [nvar] planes: the new state (not the planes of s.fields)
    double* red;                   // one reduction scalar, the bit pattern of a non-negative double
    double b[TF_MAX_TERMS], d[TF_MAX_TERMS];
    double b_last, d_last;
    int with_d;                    // 0: no estimate, red is not touched
    int pad;
};
struct TfErkArgs { TfSweepArgs s; TfErkTail x; };

struct TfVecArgs {                 // elementwise plane algebra
    int64_t n;                     // elements (nvar * plane)
    int nterms;
    int op;
    double* out;
    const double* base;
    const double* x[TF_MAX_TERMS];
    double c[TF_MAX_TERMS];
    double* red;                   // reduction target (max-norm)
    double c2[TF_MAX_TERMS];       // TF_VEC_SUM_ERR: the coefficients of the error estimate
};

struct TfPermArgs {                // natural order <-> partition-interleaved
    TfLayout L;
    const double* src;
    double* dst;
    int ncomp;                     // components handled (planes / interleave width)
    int mode;
};

struct TfGatherArgs {              // out[t] = J value table entry map[t] = node * nnz + k  (CSC assembly)
    TfLayout L;
    const double* Jv;
    const int* map;
    double* out;
    int64_t n;
    int nnz;
};

struct TfDirichletArgs {
    TfLayout L;
    double* fields;
    int n;
    const int* var;
    const int* node;               // node index inside a system (applied to all systems)
    const double* value;
};

// A few point writes passed by value (tf_poke: node assignments of a Python hook); no
// device arrays, so the launch needs no upload and no synchronisation.
#define TF_POKE_MAX 8
struct TfPokeArgs {
    TfLayout L;
    double* fields;
    int n;
    int var[TF_POKE_MAX];
    int node[TF_POKE_MAX];
    double value[TF_POKE_MAX];
};

// One level of the banded solver.  Level 1 reads its block rows from the
// Jacobian planes (A = I - c J, built on the fly); levels >= 2 read the
// explicit block-tridiagonal reduced system produced by the level below.
struct TfLevelArgs {
    TfLayout L;
    // level 1 matrix source: the Jacobian value planes; entries that do not depend on the node
    // are evaluated from the scalar parameters instead of being read (TfJUniform)
    const double* Jv;
    const double* parsca;
    const double* dx;
    double c;
    // level >= 2 matrix source: [3][b][b] planes (sub, diag, super)
    const double* Ablk;
    // right-hand side in / solution out: [B] planes
    const double* rhs;
    double* x;
    // factor storage (down direction): Ut [MP][B][B], Et [MP][B][B] planes; yt [B] planes
    double* Ut;
    double* Et;
    double* yt;
    // levels >= 2 only: stored pivot inverses [2 directions][b][b] planes and the
    // normalised ahead blocks of the upward walk [b][b] planes (downward: Ut)
    double* Dinv;
    double* Unup;
    // spike tips, SoA over chunks: see tf_kernels.h (TipLayout)
    double* tips_dn;
    double* tips_up;
    // next (coarser) level: matrix / rhs written by the assemble kernels,
    // solution read by the back-substitution
    TfLayout Lnext;
    double* Anext;
    double* rhsnext;
    const double* xnext;
    int* status;                   // != 0 when a pivot block was singular / non-finite
    // cooperative reduced-level LU: also eliminate this many columns (b spike columns,
    // +1 for a right-hand side) in the same walk; 0 = the separate column kernel does it
    int lu_cols;
    // cyclic-reduction levels (tf_coop_hip.h, tfk_cr_*): this level's and the next
    // level's buffers are in natural node order, one record per node:
    //   Ablk [node][4][b][b]  (sub, diag, super, second part of diag)
    //   rhs  [node][2][b]     (two parts, summed on load)      x [node][b]
    // next_aos: the NEXT level is stored that way (level 1 writes / reads it)
    int next_aos;
    int cr_rhs;                    // tfk_cr_factor: also eliminate the right-hand side
    double* crf;                   // [node][5][b][b]: Dinv, E, F, Ua, Lb of the eliminated node
    double* zt;                    // [node][b]: Dinv * y of the eliminated node
    // [node] + [system]: pivot order the block inversion of a node (and of the top block) used last
    // time, 3 bits per block row, 0 = natural order; tried first by the next factorisation (tf_gj_node)
    unsigned* perm;
    // last cyclic-reduction level (one chunk per system): it also inverts / applies the
    // single block that is left (what tfk_top_* do otherwise)
    int fold_top;
    // level 1 only: the spike response E of the down walk is not stored; once the separators are
    // solved, tfk_l1_fwd2 eliminates the right-hand side again with the separator above known, and
    // the back-substitution uses U alone (tfk_l1_backsub_u).  Chosen per solver (TF_RESPIKE_*).
    int respike;
    int twist;                     // ... with the down and the up walk sharing every chunk (tf_twist_h)
    // tfk_l1_fwd2_backsub (both of the above in one launch): rows of a walk's y block in the
    // workgroup's dynamic LDS, [direction][row][b][64 lanes]
    int ylds_rows;
    // level 1 below a cyclic-reduction level: the walks assemble the separator rows themselves
    // (tf_asm_side: no tips in memory, no tfk_l1_asm_* launch)
    int fuse_asm;
    // tfk_l1_fwd2_backsub of the last solve of a time step: the new state leaves instead of x,
    // upd_out = upd_base + upd_c0 x (upd_n == 1) or upd_base + (upd_c0 upd_k0 + upd_c1 x) (upd_n == 2)
    double* upd_out;
    const double* upd_base;
    const double* upd_k0;
    double upd_c0, upd_c1;
    int upd_n;
    double* topAinv;               // [b][b] planes over systems (TfTopArgs::Ainv)
    double* topx;                  // [sys][b]
    // diagnostic builds (-DTF_STAMPS): one workgroup writes s_memtime stamps here (else NULL)
    unsigned long long* stamps;
};

// Grids shorter than one stencil window (N < 2*mp + 1): the ghost cells of compilers.py:257-264 wrap
// or clamp onto nodes that are already in the window, the matrix I - cJ is small and dense.  One
// thread per system assembles it (duplicate columns summed, like csc_matrix() does), factorises it
// with partial pivoting and solves (tfk_tiny_factor / tfk_tiny_solve).
struct TfTinyArgs {
    TfLayout L;                    // one chunk per system (P == 1)
    const double* Jv;
    const double* parsca;
    const double* dx;
    double c;
    double* lu;                    // [nsys][n][n], n = N * nvar
    int* piv;                      // [nsys][n]
    const double* rhs;             // [nvar] planes
    double* x;                     // [nvar] planes
    int* status;
};

struct TfTailArgs {                // tfk_cr_tail: the last two cyclic-reduction levels of a solve in one launch
    TfLevelArgs lv[2];
};

// tfk_s_fwd / tfk_s_bwd: a whole solve of a model with b = mp * nvar <= 2 in two launches.  The plan is
// [level 1 | level 2: cyclic reduction in 256-node chunks | level 3: one chunk per system]; workgroup q
// owns chunk q of level 2, i.e. the level-1 chunks whose separators are that chunk's nodes: it walks
// them, reduces its chunk and hands its share of level 3 on -- the workgroup of a system that arrives
// last (`counter`, one per system, left at zero) solves level 3.  The second launch is the way back.
struct TfScalarArgs {
    TfLevelArgs lv[3];
    unsigned* counter;             // [nsys]
};

struct TfTopArgs {                 // final 1-node system per ensemble member
    int nsys;
    const double* A;               // [3][b][b] planes with Ptot = nsys
    const double* rhs;             // [b] planes
    double* Ainv;                  // [b][b] planes
    double* x;                     // [b] planes
    int* status;
    int aos;                       // 1: A [sys][4][b][b], rhs [sys][2][b], x [sys][b] (cyclic-reduction levels below)
};

// Level-1 spike response stored (E: mp*nvar^2 doubles per node, written by the factorisation and
// read by every back-substitution) or replaced by a second elimination of the right-hand side:
// the second form moves fewer bytes but costs a walk per solve.  It wins where E is big and the
// problem fills the GPU (config 3 x 8 members +9 %, config 5 +10 %, config 3 +1.3 %) and loses
// on scalar models (config 2 -12 %) and small grids (-5 % at 2e5 nodes): profiles/r02_ab_runs.txt.
#define TF_RESPIKE_MODEL(mp, nvar) ((mp) * (nvar) * (nvar) >= 8)
#define TF_RESPIKE_MIN_NODES 750000
// ... in twisted form while one walk direction leaves SIMDs idle (1024 SIMDs x 64 lanes)
#define TF_TWIST_MAX_CHUNKS 65536

// Level-1 factorisation walks by two wavefronts per 64 chunks and direction (tf_kernels.h, ROLE):
// one eliminates the band, the other carries the right-hand sides (the spike columns and the first
// right-hand side of the step) with the pivot blocks the first one publishes in LDS (two slots of
// (1 + mp) nvar^2 doubles per lane).  Each wavefront then fits 256 registers (the one-wavefront
// form of the film model needs 374 and keeps 100 values in AGPRs) and the two share a SIMD.
// Config 3: tfk_l1_factor_rhs 81 -> 75 us, 8 members per GPU 641 -> 600 us; the stiff model's
// slots (51 KB) leave room for three workgroups per CU only and the exchange costs more than the
// registers did: 488 -> 558 us, so blocks above 40 KB of slots keep the one-wavefront form
// (profiles/r03_ab_runs.txt, r3o).  Not for scalar models (rows are exchanged there).  The code
// object says which form it holds: the launch bound of tfk_l1_factor is 128 or 64
// (tfb::kernel_block).
#ifndef TF_L1_SPLIT_LDS
#define TF_L1_SPLIT_LDS (40 * 1024)
#endif
#define TF_L1_SPLIT_MODEL(mp, nvar) ((nvar) >= 2 && 2 * (1 + (mp)) * (nvar) * (nvar) * 64 * 8 <= TF_L1_SPLIT_LDS)

// nodes per thread of tfk_sweep_f_stage_rhs (the other sweeps: TF_SEG of the code object, 4 or 8).
// Two register windows per variable make its ghost rows twice as expensive: 8 nodes per thread
// read 152 MB where 4 read 176 MB (config 3; 43 against 51 us per launch, profiles/r02_ab_runs.txt)
#define TF_STAGE_SEG 8

// nodes per chunk of a cyclic-reduction level (one wavefront: 8 nodes x 8 lanes per round)
#define TF_CR_MAXLEN 16
// ... and of the scalar variant (b <= 2: one thread per node, 256-thread workgroups)
#define TF_CRS_MAXLEN 256
// ... and of a level that is ONE chunk per system (a 1 x 1 block's records fit the LDS twice as long)
#define TF_CRS_TOPLEN(b) ((b) == 1 ? 512 : 256)

// The node core (tf_node.h) of the device observers -- probes and recorders: what it takes to evaluate
// a model expression at the nodes of a resident state slot.  The base (first bytes) of the arguments of every
// observer kernel; the host runtime fills it in one place (tf_observer, tf_solver.h).
struct TfNodeArgs {
    TfLayout L;
    const double* fields;          // [nvar] planes: the state slot observed
    const double* helpers;         // [nh] planes
    const double* parvec;          // [npar] planes (only those flagged vector are read)
    const double* parsca;          // [npar][nsys] the solver's scalar parameters (+ the model's host constants)
    const double* dx;              // [nsys]
    const double* xcoord;          // 1 plane: x (the solver's when its model reads x, else the observer's own)
    const double* hc;              // [nhc][nsys] host constants of the observer's expressions
};

// Device probes (tf_probe.h, tf_rt_probe.cpp): reductions of model expressions over the nodes of every
// system, evaluated on a resident state slot.  tfk_probe_partial: grid (nsys * nblk, nseg), one thread per
// segment of TF_PROBE_SEG nodes of a level-1 chunk, one partial per workgroup, probe and system;
// tfk_probe_final: grid (nsys), reduces the partials of its system in a fixed order and writes row `row`
// of the ring.  Reductions (codegen.PROBE_REDUCTIONS: same order):
#define TF_PROBE_SUM 0
#define TF_PROBE_MEAN 1
#define TF_PROBE_INTEGRAL 2
#define TF_PROBE_MAX 3
#define TF_PROBE_MIN 4
#define TF_PROBE_ARGMAX 5
#define TF_PROBE_ARGMIN 6
#define TF_PROBE_KINDS 7
// nodes per thread of tfk_probe_partial: one thread per whole chunk left most of the GPU idle (config 3:
// 31 250 chunks of 32 nodes, 14.8 us for 24 MB); segments of 8 as in the F sweep (TF_SEG)
#define TF_PROBE_SEG 8
struct TfProbeArgs : TfNodeArgs {
    double* partial;               // [nsys][nprobe][nseg * nblk] (value, natural index) pairs
    double* ends;                  // [nsys][nprobe][2]: f at natural nodes 0 and N-1 (integral)
    int nblk;                      // workgroups of tfk_probe_partial per system and segment row
    int nseg;                      // segments of TF_PROBE_SEG nodes per chunk
    int row;                       // row of the ring this launch writes (by value: the host counts)
    int capacity;                  // rows of the ring
    double* ring;                  // [capacity][nsys][nprobe]
};

// Device recorders (tf_record.h, tf_rt_record.cpp): decimated space-time series of model expressions.
// Column j of a recorder covers the bin of natural nodes start + j*step ... min(start + (j+1)*step, stop) - 1
// of every system; tfk_record evaluates expression `which` of the record block on a resident state slot
// and stores row `row`, [nsys][ncols], of the recorder's ring.  Pools:
#define TF_REC_SAMPLE 0            // the expression at the bin's first node
#define TF_REC_MAX 1               // over the bin's nodes, NaN as numpy has it (tf_probe_combine)
#define TF_REC_MIN 2
#define TF_REC_MEAN 3              // sum in a fixed order / the bin's node count
// threads of a workgroup of tfk_record; `split` of them share a bin (a power of two <= TF_REC_BLOCK)
#define TF_REC_BLOCK 256
struct TfRecordArgs : TfNodeArgs {
    int which;                     // expression of the record block (tf_eval_record's first argument)
    int pool;                      // TF_REC_*
    int start, stop, step;         // the window of nodes (slice.indices(N), step >= 1)
    int ncols;                     // ceil((stop - start) / step)
    int split;                     // threads per bin
    int part;                      // nodes per thread = ceil(step / split)
    int nblk;                      // workgroups per system
    int row;                       // row of the ring this launch writes (by value: the host counts, and wraps)
    int capacity;                  // rows of the ring (both halves)
    double* ring;                  // [capacity][nsys][ncols]
};

// Device statistics (tf_stat.h, tf_rt_stat.cpp): per-node statistics over time of model expressions.
// tfk_stat evaluates expression `which` of the statistic block at every node of a resident state slot and
// folds the value, sample k (1, 2, ...) taken at time t, into the statistic's accumulator planes.  The
// planes have the solver's own partition-interleaved layout (TfLayout: node i of chunk p of system e at
// tf_idx(L, e * P + p, i)), so a thread updates the elements of the nodes it walks and no others.  Grid
// and walk as tfk_probe_partial: (nsys * nblk, nseg), one thread per segment of TF_PROBE_SEG nodes.
// Kinds (statistics.STATISTIC_KINDS: same order) and their planes:
#define TF_STAT_MEAN 0             // [0] running mean m_k = m_{k-1} + (v_k - m_{k-1}) / k
#define TF_STAT_VAR 1              // [0] running mean, [1] M2_k = M2_{k-1} + (v_k - m_{k-1}) * (v_k - m_k)
#define TF_STAT_MAX 2              // [0] the extremum, NaN as numpy has it (tf_node_extremum)
#define TF_STAT_MIN 3
#define TF_STAT_ARGMAX 4           // [0] the extremum, [1] t of the first sample that attained it (the first
#define TF_STAT_ARGMIN 5           //     NaN's t wins and stays)
#define TF_STAT_KINDS 6
static inline int tf_stat_planes(int kind) {
    return kind == TF_STAT_VAR || kind == TF_STAT_ARGMAX || kind == TF_STAT_ARGMIN ? 2 : 1;
}
struct TfStatArgs : TfNodeArgs {
    int which;                     // expression of the statistic block (tf_eval_stat's first argument)
    int kind;                      // TF_STAT_*
    int nblk;                      // workgroups per system and segment row
    int nseg;                      // segments of TF_PROBE_SEG nodes per chunk
    double k;                      // number of this sample, 1 for the first: it is written, nothing is read
    double t;                      // time of this sample (argmax / argmin)
    double* acc;                   // [tf_stat_planes(kind)] planes
};

// Device spectra (tf_spectrum.h, tf_rt_spectrum.cpp): Fourier amplitudes of model expressions.  Row of a
// spectrum: c[i] = sum over the natural nodes g of v_g * exp(-2 pi i m_i g / N), v the expression `which`
// of the spectrum block on a resident state slot, m_i the modes of the spectrum (a device buffer of the
// handle: the code object does not know them).  tfk_spectrum_partial: grid (nsys * nblk, nseg), one thread
// per segment of TF_PROBE_SEG nodes as tfk_probe_partial, one (re, im) pair per workgroup, mode and
// system; tfk_spectrum_final: grid (nsys), reduces the partials of its system in a fixed order and writes
// row `row` of the ring.
// Modes of one spectrum.  The tables of a workgroup of tfk_spectrum_partial in LDS are the step twiddles
// [TF_PROBE_SEG][modes] and the sums of its four wavefronts [4][modes], complex doubles: 192 bytes per
// mode, 12 KiB at 64.  A CU holds 8 workgroups of 256 threads (32 wavefronts) and 160 KiB of LDS: at 64
// modes the tables take 96 KiB and the registers decide how many workgroups are resident, at 128 they
// would take 192 KiB and the LDS would.
#define TF_SPEC_MAX_MODES 64
struct TfSpectrumArgs : TfNodeArgs {
    int which;                     // expression of the spectrum block (tf_eval_spectrum's first argument)
    int nmodes;                    // 1 ... TF_SPEC_MAX_MODES
    int nblk;                      // workgroups of tfk_spectrum_partial per system and segment row
    int nseg;                      // segments of TF_PROBE_SEG nodes per chunk
    int row;                       // row of the ring this launch writes (by value: the host counts)
    int capacity;                  // rows of the ring
    const int* modes;              // [nmodes], each 0 ... N / 2
    double* partial;               // [nsys][nmodes][nseg * nblk] (re, im) pairs
    double* ring;                  // [capacity][nsys][nmodes] (re, im) pairs
};

// Device extrema (tf_extrema.h, tf_rt_extrema.cpp): the crests or troughs of a model expression, a row of
// variable length in node order.  Node g is an extremum of kind max iff v[g-1] < v[g] > v[g+1] (strictly;
// min: both reversed) and v[g] is finite and beyond `threshold` (v > threshold, min: v < threshold; the host
// passes -inf / +inf for "no threshold"); the neighbours wrap on a periodic grid, nodes 0 and N-1 of any
// other grid are never extrema.  tfk_extrema_count: grid (nsys * nblk), thread = chunk, the extrema of every
// chunk and of every workgroup; tfk_extrema_write: same grid, an exclusive integer scan of those counts gives
// every chunk its place in the row, the walk is repeated and the first max_count entries are stored.
// Row of the ring, per system: [0] the number of extrema found (may exceed max_count), then max_count
// entries (g, v[g-1], v[g], v[g+1]); all doubles (node indices and counts are exact).
#define TF_EXT_MAX 0
#define TF_EXT_MIN 1
#define TF_EXT_MAX_COUNT 8192
struct TfExtremaArgs : TfNodeArgs {
    int which;                     // expression of the extrema block (tf_eval_extrema's first argument)
    int kind;                      // TF_EXT_MAX / TF_EXT_MIN
    int max_count;                 // entries of a row, 1 ... TF_EXT_MAX_COUNT
    int nblk;                      // workgroups per system
    int row;                       // row of the ring this launch writes (by value: the host counts)
    int capacity;                  // rows of the ring
    double threshold;              // -inf (max) / +inf (min): none
    int* counts;                   // [nsys][nblk * 256] extrema per chunk
    int* sums;                     // [nsys][nblk] extrema per workgroup
    double* ring;                  // [capacity][nsys][1 + 4 * max_count]
};

// Device histograms (tf_histogram.h, tf_rt_histogram.cpp): the distribution of the values of a model
// expression over the window nodes start, start + step, ... < stop of every system.  Bin i counts
// edges[i] <= v < edges[i + 1], the last bin also v == edges[nbins]; three more counters take what is
// outside: v < edges[0], v > edges[nbins] and v != v.  A row is nbins + 3 counts, which sum to the number of
// window nodes.  tfk_hist_partial: grid (nsys * nblk, nseg), one thread per segment of TF_PROBE_SEG nodes as
// tfk_probe_partial, counts in unsigned 32-bit integers in LDS, one set of nbins + 3 per workgroup leaves
// with plain stores; tfk_hist_final: grid (nsys, ceil((nbins + 3) / 64)), 1024 threads, sums the sets of its
// system and writes row `row` of the ring as doubles (exact: a count is below 2^53).  Integers throughout: any order gives the same row.
// These two kernels are not in the kernel table below: the runtime resolves them by name
// (tfb::kernel_lookup) in a code object of kind "histogram".
#define TF_HIST_MAX_BINS 256
struct TfHistArgs : TfNodeArgs {
    int which;                     // expression of the histogram block (tf_eval_hist's first argument)
    int nbins;                     // 1 ... TF_HIST_MAX_BINS
    int nblk;                      // workgroups of tfk_hist_partial per system and segment row
    int nseg;                      // segments of TF_PROBE_SEG nodes per chunk
    int row;                       // row of the ring this launch writes (by value: the host counts)
    int capacity;                  // rows of the ring
    int start, stop, step;         // the window of nodes (slice.indices(N), step >= 1)
    int pad;
    const double* edges;           // [nbins + 1], finite and strictly increasing
    unsigned* partial;             // [nsys][nseg * nblk][nbins + 3]
    double* ring;                  // [capacity][nsys][nbins + 3]
};
// Device hooks (tf_hook.h, tf_rt_hook.cpp): a program of statements fields[var][target] = expression that
// WRITES a resident state, executed in the order given; every statement sees the assignments of the ones
// before it.  A point statement assigns one node (and may read other nodes through at()), a window
// statement the nodes start, start + step, ... < stop with the expression at the node being assigned.
// Kinds, targets and at() reads are static tables of the generated block (codegen.lower_hooks); a launch
// takes one maximal run of consecutive statements of one kind: first ... first + count - 1.
//   tfk_hook_window: grid (nsys * nblk, nsg), 256 threads: thread x of workgroup blk walks the rows of
//     segment sg0 + blockIdx.y (TF_PROBE_SEG rows) of chunk p0 + blk * 256 + x, of the chunks p0 ... p1 - 1:
//     the chunks and rows the union of the run's windows touches.
//   tfk_hook_points: grid (ceil(nsys / 64)), 64 threads, one thread per system.
// `hc` of the base is the set of host constants of this application (the call before the step or the one
// after it): t reaches the kernels through it and through nothing else, so a captured launch replays with
// the t uploaded last.  These two kernels are not in the kernel table below: the runtime resolves them by
// name (tfb::kernel_lookup) in a code object of kind "hook".
#define TF_HOOK_POINT 0
#define TF_HOOK_WINDOW 1
struct TfHookArgs : TfNodeArgs {
    double* out;                   // [nvar] planes: the planes of `fields` (the program assigns in place)
    int first, count;              // the run: statements first ... first + count - 1
    int p0, p1;                    // window runs: the chunks p0 ... p1 - 1 of every system ...
    int sg0, nblk;                 // ... from segment sg0 on; workgroups per system and segment row
};
// (passed by value to kernels of code objects the host did not compile: the bytes are the contract)
// (the base comes first and the members follow in their order: the sizes pin the bytes)
static_assert(sizeof(TfHookArgs) == 128, "TfHookArgs changed its layout");
static_assert(sizeof(TfHistArgs) == 160, "TfHistArgs changed its layout");
static_assert(sizeof(TfNodeArgs) == 96, "TfNodeArgs changed its layout");
static_assert(sizeof(TfProbeArgs) == 136, "TfProbeArgs changed its layout");
static_assert(sizeof(TfRecordArgs) == 152, "TfRecordArgs changed its layout");
static_assert(sizeof(TfStatArgs) == 136, "TfStatArgs changed its layout");
static_assert(sizeof(TfSpectrumArgs) == 144, "TfSpectrumArgs changed its layout");
static_assert(sizeof(TfExtremaArgs) == 152, "TfExtremaArgs changed its layout");

// Kernel table: index = launch id used by the runtime, name = entry point in a code object of the
// model: the ids before TFK_PROBE_PARTIAL in the model's own (tf_entry_hip.h), an observer's from there
// on in the code object of its kind (tf_probe.h ...).  A module resolves the range of its kind
// (tfb::module_resolve).  New entries go at the end: the launch ids and the timing-mask bits of the
// others stay put.
enum TfKernel {
    TFK_SWEEP_F = 0, TFK_SWEEP_FJ, TFK_SPMV, TFK_VEC, TFK_VEC_MAXABS, TFK_PERM, TFK_DIRICHLET,
    TFK_L1_FACTOR, TFK_L1_SOLVE, TFK_L1_ASM_MAT, TFK_L1_ASM_RHS, TFK_L1_BACKSUB,
    TFK_BT_LU, TFK_BT_SPIKE, TFK_BT_RHS, TFK_BT_ASM_MAT, TFK_BT_ASM_RHS, TFK_BT_BACKSUB,
    TFK_TOP_FACTOR, TFK_TOP_SOLVE, TFK_BERR, TFK_DIFFNORM, TFK_L1_FACTOR_RHS, TFK_SWEEP_F_STAGE,
    TFK_CR_FACTOR, TFK_CR_FWD, TFK_CR_BWD, TFK_POKE, TFK_SWEEP_FJ_THETA, TFK_SWEEP_FJ_BDF2, TFK_GATHER,
    TFK_SWEEP_F_STAGE_RHS, TFK_L1_FWD2, TFK_L1_BACKSUB_U, TFK_CR_TAIL, TFK_L1_FWD2_BACKSUB, TFK_TINY_FACTOR, TFK_TINY_SOLVE,
    TFK_S_FWD, TFK_S_BWD, TFK_SWEEP_F_STAGE_RHS_N, TFK_L1_SOLVE_CR, TFK_L1_FWD2_BACKSUB_CR, TFK_SWEEP_F_STAGE_RHS_MON,
    TFK_PROBE_PARTIAL, TFK_PROBE_FINAL,
    TFK_RECORD, TFK_COUNT          // (from TFK_RECORD on: TF_KERNEL_NAMES_RECORD)
};
#define TF_KERNEL_NAMES { \
    "tfk_sweep_f", "tfk_sweep_fj", "tfk_spmv", "tfk_vec", "tfk_vec_maxabs", "tfk_perm", "tfk_dirichlet", \
    "tfk_l1_factor", "tfk_l1_solve", "tfk_l1_asm_mat", "tfk_l1_asm_rhs", "tfk_l1_backsub", \
    "tfk_bt_lu", "tfk_bt_spike", "tfk_bt_rhs", "tfk_bt_asm_mat", "tfk_bt_asm_rhs", "tfk_bt_backsub", \
    "tfk_top_factor", "tfk_top_solve", "tfk_berr", "tfk_diffnorm", "tfk_l1_factor_rhs", "tfk_sweep_f_stage", \
    "tfk_cr_factor", "tfk_cr_fwd", "tfk_cr_bwd", "tfk_poke", "tfk_sweep_fj_theta", "tfk_sweep_fj_bdf2", \
    "tfk_gather", "tfk_sweep_f_stage_rhs", "tfk_l1_fwd2", "tfk_l1_backsub_u", "tfk_cr_tail", \
    "tfk_l1_fwd2_backsub", "tfk_tiny_factor", "tfk_tiny_solve", "tfk_s_fwd", "tfk_s_bwd", "tfk_sweep_f_stage_rhs_n", \
    "tfk_l1_solve_cr", "tfk_l1_fwd2_backsub_cr", "tfk_sweep_f_stage_rhs_mon", \
    "tfk_probe_partial", "tfk_probe_final" }
// ... continued: the kernels of the recorders (ids TFK_RECORD ...), a table of their own
#define TF_KERNEL_NAMES_RECORD { "tfk_record" }
// ... and the launch ids after TFK_COUNT, with a table of their own as well: the kernel of the statistics.
// TFK_TOTAL is the number of kernels of the table: what the runtime sizes its per-kernel arrays by.
// After it, the kernels of the spectra (TF_KERNEL_NAMES_SPECTRUM), then those of the extrema
// (TF_KERNEL_NAMES_EXTREMA).
enum TfKernelMore { TFK_STAT = TFK_COUNT, TFK_SPECTRUM_PARTIAL, TFK_SPECTRUM_FINAL,
                    TFK_EXTREMA_COUNT, TFK_EXTREMA_WRITE, TFK_TOTAL };
#define TF_KERNEL_NAMES_STAT { "tfk_stat" }
#define TF_KERNEL_NAMES_SPECTRUM { "tfk_spectrum_partial", "tfk_spectrum_final" }
#define TF_KERNEL_NAMES_EXTREMA { "tfk_extrema_count", "tfk_extrema_write" }
static inline const char* tf_kernel_entry(int kernel) {
    static const char* const base[] = TF_KERNEL_NAMES;
    static const char* const rec[] = TF_KERNEL_NAMES_RECORD;
    static const char* const stat[] = TF_KERNEL_NAMES_STAT;
    static_assert(sizeof(base) / sizeof(base[0]) == TFK_RECORD, "TF_KERNEL_NAMES and TfKernel differ");
    static_assert(sizeof(rec) / sizeof(rec[0]) == TFK_COUNT - TFK_RECORD, "TF_KERNEL_NAMES_RECORD and TfKernel differ");
    static const char* const spec[] = TF_KERNEL_NAMES_SPECTRUM;
    static_assert(sizeof(stat) / sizeof(stat[0]) == TFK_SPECTRUM_PARTIAL - TFK_STAT, "TF_KERNEL_NAMES_STAT and TfKernelMore differ");
    static const char* const ext[] = TF_KERNEL_NAMES_EXTREMA;
    static_assert(sizeof(spec) / sizeof(spec[0]) == TFK_EXTREMA_COUNT - TFK_SPECTRUM_PARTIAL, "TF_KERNEL_NAMES_SPECTRUM and TfKernelMore differ");
    static_assert(sizeof(ext) / sizeof(ext[0]) == TFK_TOTAL - TFK_EXTREMA_COUNT, "TF_KERNEL_NAMES_EXTREMA and TfKernelMore differ");
    static_assert(TFK_TOTAL <= 64, "the timing mask has one bit per kernel");
    if (kernel < 0 || kernel >= TFK_TOTAL) return "";
    if (kernel >= TFK_EXTREMA_COUNT) return ext[kernel - TFK_EXTREMA_COUNT];
    if (kernel >= TFK_SPECTRUM_PARTIAL) return spec[kernel - TFK_SPECTRUM_PARTIAL];
    if (kernel >= TFK_STAT) return stat[kernel - TFK_STAT];
    return kernel < TFK_RECORD ? base[kernel] : rec[kernel - TFK_RECORD];
}
