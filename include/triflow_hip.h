/* libtriflow_hip -- C ABI of the MI355X-native triflow hot path.
 *
 * Drop-in boundary.  Plain pointers and sizes only; all
 * device memory is owned by the library, host pointers are borrowed for the
 * duration of a call.  Every function returns 0 on success, non-zero on error
 * (text via tf_last_error()); the Python host side raises RuntimeError from it,
 * which is what the reference's Simulation turns into status = 'failed'
 * (triflow/core/simulation.py:259-261).
 *
 * Reference interfaces replaced (paths relative to the reference tree):
 *   seam #1  compiler plugin  compiler(model) -> (F_function, J_function)
 *            triflow/core/model.py:299-311, callables invoked as
 *            _ufunc(x, *dep_vars, *help_funcs, *pars, periodic)
 *            triflow/core/routines.py:37-45, 82-91
 *            -> tf_model_create, tf_solver_create, tf_set_*, tf_eval, tf_get_F, tf_get_J
 *   seam #2  scheme plugin    scheme(t, fields, dt, pars, hook) -> (t, fields)
 *            triflow/core/schemes.py:101-174 (ROW_general), 523-559 (Theta)
 *            -> tf_step_theta, tf_step_row, tf_step_bdf2, tf_step_erk (BDF-2 and the explicit
 *               Runge-Kutta steps are new)
 *   seam #3  linear-solver injection  Theta(model, solver=callable(A, b) -> x)
 *            triflow/core/schemes.py:518-521, 557
 *            -> tf_factor, tf_solve
 *
 * Threading: calls on one solver are not thread-safe; different solvers are
 * independent (one HIP stream each).
 */
#ifndef TRIFLOW_HIP_H
#define TRIFLOW_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct tf_model tf_model;
typedef struct tf_solver tf_solver;

/* Constants of one compiled model (produced by triflow_amd.codegen). */
typedef struct tf_model_spec {
    int32_t nvar;         /* dependent variables                                   */
    int32_t nh;           /* help functions                                        */
    int32_t npar;         /* physical parameters (without 'periodic')              */
    int32_t mp;           /* ghost width: stencil window is 2*mp+1 nodes           */
    int32_t nnz;          /* structurally non-null Jacobian entries per node       */
    int32_t seg;          /* nodes per thread of the stencil sweep                 */
    int32_t sweep_block;  /* workgroup size of the stencil sweep                   */
    int32_t uses_x;       /* the expressions read the coordinate x                 */
    uint32_t parvec_mask; /* bit k set: parameter k is a per-node array            */
} tf_model_spec;

typedef struct tf_solver_opts {
    int32_t m1;           /* chunk length of the first solver level (0 = by problem
                             size: 4 ... 32 nodes)                                  */
    int32_t m_upper;      /* chunk length of the reduced levels (0 = default: 6 for
                             the chunk walks, 16 = the maximum for cyclic reduction) */
    int32_t nstate;       /* resident state slots                   (0 = default 3) */
    int32_t refine;       /* refinement sweeps per solve; 0 = none, -1 = automatic:
                             measure the backward error of the first solve after
                             each factorisation and polish only if it is > 1e-11   */
    int32_t device;       /* HIP device ordinal (-1 = current)                      */
    int32_t berr_every;   /* refine = -1: after the first factorisations (and whenever c
                             moves by > 10 %) the backward error is re-measured on every
                             berr_every-th factorisation (n > 0: that interval, 1 = always;
                             0 = default: 8, doubling up to 64 while the checks read
                             rounding level, back to 8 as soon as one does not); halfway
                             between two checks a Rosenbrock step measures it in passing  */
    int32_t reserved;     /* must be 0 */
} tf_solver_opts;

const char* tf_last_error(void);
int tf_runtime_info(int32_t* is_device_build, int32_t* device_count);
/* current HIP device of the calling thread: code objects are loaded, and solvers
 * created with device = -1 live, on it */
int tf_set_device(int32_t ordinal);

/* code object = gfx950 .hsaco image built from the generated per-model source.
 *
 * What a code object must hold.  A model's (tf_model_create): the solver's kernels of the kernel table
 * (tf_kernel_name), which are the names before "tfk_probe_partial", and the two by-name kernels of the
 * explicit schemes where those are used.  An observer's (tf_probe_create ... tf_histogram_create): the
 * kernels of its own kind -- tfk_probe_partial / tfk_probe_final, tfk_record, tfk_stat,
 * tfk_spectrum_partial / tfk_spectrum_final, tfk_extrema_count / tfk_extrema_write, or (by name)
 * tfk_hist_partial / tfk_hist_final -- and none of the solver's.  A create call resolves exactly these
 * names and fails with "kernel missing from code object: NAME" when one is absent, so a code object of
 * another kind is refused there; what else the image holds is not looked at (an image with every kernel
 * of the table in it loads everywhere). */
int tf_model_create(const tf_model_spec* spec, const void* code_object, size_t code_size,
                    tf_model** out);
/* Second build of the same code object (lower optimisation level): the kernels whose bit
 * is set in kernel_mask (index = tf_kernel_name) are launched from it.  The compiler plugin
 * uses it for kernels that spill registers to scratch at -O3 (wide models). */
int tf_model_add_alternate(tf_model* model, const void* code_object, size_t code_size,
                           uint64_t kernel_mask);
void tf_model_destroy(tf_model* model);

/* nsys independent systems (ensemble members) of N nodes each share one solver */
int tf_solver_create(tf_model* model, int64_t N, int32_t nsys, int32_t periodic,
                     const tf_solver_opts* opts, tf_solver** out);
void tf_solver_destroy(tf_solver* solver);
int tf_solver_describe(tf_solver* solver, int32_t* nlevels, int32_t* chunks /*[nlevels]*/,
                       int32_t max_levels, int64_t* device_bytes);

/* ---- inputs.  Arrays are [nsys][N] in natural node order. ------------------- */
int tf_set_state(tf_solver*, int32_t slot, int32_t first_var, int32_t nvars, const double* host);
int tf_get_state(tf_solver*, int32_t slot, int32_t first_var, int32_t nvars, double* host);
int tf_set_state_flat(tf_solver*, int32_t slot, const double* uflat /*[nsys][N*nvar]*/);
int tf_get_state_flat(tf_solver*, int32_t slot, double* uflat);
int tf_copy_state(tf_solver*, int32_t src_slot, int32_t dst_slot);
int tf_set_helpers(tf_solver*, int32_t first, int32_t count, const double* host);
int tf_set_param_scalar(tf_solver*, int32_t k, const double* values /*[nsys]*/);
int tf_set_param_vector(tf_solver*, int32_t k, const double* host /*[nsys][N]*/);
int tf_set_dx(tf_solver*, const double* dx /*[nsys]*/);
int tf_set_x(tf_solver*, const double* x /*[nsys][N]*/);
/* declarative Dirichlet hook: U[var][node] = value (node < 0 counts from the end),
 * applied where the reference schemes call hook() */
int tf_set_dirichlet(tf_solver*, int32_t n, const int32_t* var, const int64_t* node,
                     const double* value);

/* time-dependent boundary values: `before` is applied where the reference calls
 * hook(t, ...) at the start of a step, `after` where it calls hook(t + dt, ...)
 * (either may be NULL = unchanged); same entries as the last tf_set_dirichlet */
int tf_set_dirichlet_values(tf_solver*, const double* before, const double* after);
/* n point writes state[var[i]][node[i]] = value[i] (negative nodes count from the end) into a
   resident slot, for every system: what a Python hook like the reference README's
   ``fields.U[0] = 1`` does, without moving the state over PCIe.                         */
int tf_poke(tf_solver*, int32_t slot, int32_t n, const int32_t* var, const int64_t* node,
            const double* value);
/* ... and the values of single nodes, out[i * nsys + system] */
int tf_peek(tf_solver*, int32_t slot, int32_t n, const int32_t* var, const int64_t* node,
            double* out);

/* ---- seam #1: F / J evaluation on the resident state ----------------------- */
int tf_eval(tf_solver*, int32_t slot, int32_t with_j);
/* `reps` back-to-back sweeps between two HIP events on the solver's stream */
int tf_eval_repeat(tf_solver*, int32_t slot, int32_t with_j, int32_t reps, double* total_ms);
/* F of the last tf_eval.  After a step function the F buffer is unspecified: the fused sweeps of
 * the theta and BDF-2 steps fold F into the right-hand side they write and leave the buffer alone,
 * a ROW step leaves dt*F there.  Call tf_eval before tf_get_F. */
int tf_get_F(tf_solver*, double* F /*[nsys][N*nvar], F[node*nvar+eq]*/);
int tf_get_J(tf_solver*, double* Jvals /*[nsys][N][nnz], reference pattern order*/);

/* the Jacobian values in the order of a caller's index list, uploaded once: out[t] = value-table
 * entry map[t] = node * nnz + k of system 0 -- the data array of the csc_matrix that the
 * reference's J function returns (compilers.py:303-331), gathered on the device */
int tf_set_csc_map(tf_solver*, const int32_t* map, int64_t n);
int tf_get_J_mapped(tf_solver*, double* out /*[n]*/);

/* Declares that no Jacobian entry of the model depends on the state or on the node (constant-
 * coefficient linear models such as the reference README's "k * dxxU - c * dxU"; codegen marks
 * the entries, spec["j_uniform"]).  The matrix I - c J of a step then only depends on c, the
 * scalar parameters and dx: the step functions keep the factorisation while those are unchanged
 * and only solve -- where the reference factorises in every step (schemes.py:148-149, 557).
 * Any tf_set_param_scalar / tf_set_param_vector / tf_set_dx invalidates it. */
int tf_set_constant_jacobian(tf_solver*, int32_t on);

/* ---- seam #3: (I - c J) x = b with the Jacobian of the last tf_eval -------- */
int tf_factor(tf_solver*, double c);
int tf_solve(tf_solver*, const double* rhs_flat /*[nsys][N*nvar]*/, double* x_flat);
int tf_matvec(tf_solver*, const double* v_flat, double* y_flat);     /* y = J @ v */

/* ---- seam #2: one time step, state slot src -> slot dst --------------------- */
int tf_step_theta(tf_solver*, int32_t src, int32_t dst, double dt, double theta);
/* alpha, gamma: [s][s] row major; b, b_pred: [s] (b_pred may be NULL);
 * err_out (may be NULL) receives ||U - U_pred||_inf, one scalar over all systems;
 * hook_after: apply the Dirichlet list to the result (fixed-step __call__).
 * The estimate is never finite when a state is not: NaN wins the maximum, as in np.linalg.norm.
 * With a NaN in the input state of one system, tf_step_row fails (non-zero return: the
 * factorisation meets a non-finite pivot block); tf_read_err after tf_step_row_queued returns
 * NaN, and the next call that synchronises (tf_get_state, tf_sync) fails */
int tf_step_row(tf_solver*, int32_t src, int32_t dst, double dt, int32_t s,
                const double* alpha, const double* gamma, const double* b,
                const double* b_pred, int32_t hook_after, double* err_out);
/* Explicit Runge-Kutta step (new; the reference has none).  a: [s][s] row major, strictly lower
 * triangular; b: [s]; d: [s] or NULL, the weights of the error estimate, d = b - b_err with b_err the
 * weights of the embedded lower-order solution, formed on the host; 1 <= s <= 8.  No Jacobian is
 * evaluated and nothing is factorised or solved: the factorisation in memory and its counters are left
 * alone.  The arithmetic, without contraction:
 *   k_i  = dt * F(U + (((a_i0*k_0) + a_i1*k_1) + ...))        i = 0 ... s-1
 *   U+   = U + (((b_0*k_0) + b_1*k_1) + ...)
 *   err  = max over nodes, variables and systems of |((d_0*k_0) + d_1*k_1) + ...|      (NaN wins)
 * A term whose coefficient is exactly 0.0 is left out of its sum in all three lines, so a non-finite
 * k_j does not reach a sum it is no part of; a stage without terms evaluates F(U).  err_out (may be NULL)
 * receives err when d is given, else 0.  hook_after: the Dirichlet list is applied to the result.
 * src != dst.  The last stage runs in one pass with the update and the estimate (tfk_sweep_f_erk_last)
 * or, TRIFLOW_ERK_FUSED=0 when the solver is created, as a stage sweep followed by tfk_vec and
 * tfk_vec_maxabs: the same bits either way. */
int tf_step_erk(tf_solver*, int32_t src, int32_t dst, double dt, int32_t s,
                const double* a, const double* b, const double* d, int32_t hook_after,
                double* err_out);
/* which form the explicit steps of this solver take (fused: 1 / 0, fixed when the solver is created),
 * how many tf_step_erk calls it has served, and how many of them ran the fused last stage */
int tf_erk_info(tf_solver*, int32_t* fused, int64_t* steps, int64_t* fused_steps);
/* linearly implicit BDF-2 (new, scheme protocol of schemes.py:523-559); the history U_{n-1}
 * is the solver's own: for a caller that owns the solver and steps one trajectory on it */
int tf_step_bdf2(tf_solver*, int32_t src, int32_t dst, double dt);
int tf_bdf2_reset(tf_solver*);
/* the same step for scheme objects that share a solver: `owner` (non-zero) names the history
 * buffer of one scheme instance, `continuing` != 0 says that slot `src` holds the state that
 * owner's previous step produced; otherwise the step restarts in backward-Euler form */
int tf_step_bdf2_owned(tf_solver*, int32_t src, int32_t dst, double dt, int64_t owner,
                       int32_t continuing);
int tf_bdf2_release(tf_solver*, int64_t owner);      /* frees that history buffer */
/* the same step with the history in a state slot of the caller's: `prev` holds U_{n-1}, or is -1
 * (first step, or the step size changed: backward-Euler form).  Nothing is copied.  With Dirichlet
 * values set, `src` is the next step's history and must hold the *hooked* state (the reference's
 * schemes keep the hooked copy): unless a step of this solver left it so, the boundary values are
 * written into slot `src` in place -- the one step function that modifies its input slot. */
int tf_step_bdf2_from(tf_solver*, int32_t src, int32_t dst, int32_t prev, double dt);
/* tf_step_row with the embedded error estimate left on the device, in reduction slot `err_slot`
 * (1, 2 or 3), until tf_read_err fetches it (blocking; the failure flag is looked at as well).  For a
 * driver of the adaptive schemes (triflow/core/schemes.py:176-238) that queues the first trial of the
 * next call before it reads the estimate of the step it is about to return: the host's decision
 * overlaps with the GPU's next step.  b_pred is required. */
int tf_step_row_queued(tf_solver*, int32_t src, int32_t dst, double dt, int32_t stages,
                       const double* alpha, const double* gamma, const double* b,
                       const double* b_pred, int32_t hook_after, int32_t err_slot);
int tf_read_err(tf_solver*, int32_t err_slot, double* err_out);
/* One trial of the reference's universal step-doubling controller (schemes.py:33-66; it wraps
 * every scheme a Simulation builds, simulation.py:190-197) without a host round trip per
 * sub-step: a coarse step m*dt (src -> coarse), `nfine` fine steps dt (src -> tmp -> dst ...,
 * nfine even: the last one lands in dst; the reference's loop bound is the literal 10) and the
 * norm of their difference, queued back to back; the call returns when the norms are on the
 * host: err_out[system] = max_var ||coarse - dst||_ord / (m*m - 1), ord = 2 or 0 (max).
 * The Dirichlet list of the solver is applied as in the single steps. */
enum { TF_SCHEME_THETA = 0, TF_SCHEME_ROW = 1 };
typedef struct tf_scheme {
    int32_t kind;            /* TF_SCHEME_THETA / TF_SCHEME_ROW */
    int32_t stages;          /* ROW: s */
    double theta;            /* Theta */
    const double* alpha;     /* ROW: [s][s] */
    const double* gamma;     /* ROW: [s][s] */
    const double* b;         /* ROW: [s] */
    int32_t hook_after;      /* ROW: the extra hook call of the fixed-step __call__ */
    int32_t reserved;
} tf_scheme;
int tf_step_doubling(tf_solver*, int32_t src, int32_t dst, int32_t tmp, int32_t coarse, double dt,
                     int32_t m, int32_t nfine, const tf_scheme* scheme, int32_t ord, double* err_out);
/* ||state[a] - state[b]||_ord of every dependent variable, out[nsys][nvar]; ord = 2
 * or 0 (max norm): the error estimate of the step-doubling wrapper
 * (schemes.py:41-44) without bringing the fields to the host.  NaN propagates as in
 * np.linalg.norm, for both values of ord: a NaN difference at any node makes that variable's
 * and system's norm NaN (the maximum lets NaN win and keeps it), and only that one.  The maximum
 * norm is exact (the bits of np.abs(a - b).max()); the 2-norm is within (N + 2) * 2^-53, relative */
int tf_diff_norm(tf_solver*, int32_t slot_a, int32_t slot_b, int32_t ord, double* out);

/* componentwise backward error max|b-Ax|/(|x|+|cJ||x|+|b|) measured on the first
 * solve after the last factorisation (refine = -1), and whether it triggered
 * refinement */
int tf_backward_error(tf_solver*, double* omega, int32_t* refined);

/* Between two explicit (synchronising) checks every step measures the backward error of its
 * factorisation's first solve at one node of every level-1 chunk, a different node in every step (no
 * synchronisation; a Rosenbrock step inside the launch of stage 1's right-hand side, a Theta / BDF-2
 * step in a small launch of its own; with refine = -2 there are no explicit checks).  The worst value
 * since the last synchronising call is looked at there (above 1e-11: the next factorisation is
 * checked and refined; above 1e-6: RuntimeError).  This reads it without resetting / raising. */
int tf_monitor_error(tf_solver*, double* worst);
/* counters since the solver was created: factorisations made (a step of a constant-matrix model
 * that finds its factorisation in memory -- one of two, keyed by c -- makes none), backward-error
 * checks that waited for the device, and factorisations that were redone on longer chunks because
 * the first attempt lost accuracy */
int tf_solver_counters(tf_solver*, int64_t* factorisations, int64_t* checks, int64_t* replans);
/* F+J sweeps since the solver was created.  The planes of the value table that hold node-independent
 * entries (spec["j_uniform"]: functions of dx, the scalar parameters and constants) are written by the
 * first sweep after tf_set_param_scalar / tf_set_param_vector / tf_set_dx and left alone by the following
 * ones (`lean`), their values being the same; the table tf_get_J reads is complete at all times.
 * `full` counts the sweeps that wrote every plane (all of them with TRIFLOW_J_UNIFORM_ONCE=0). */
int tf_jacobian_sweeps(tf_solver*, int64_t* full, int64_t* lean);
/* the workgroup size a kernel of the model's code object was built for (tfk_l1_factor*: 128 when
 * the factorisation walks are split over two wavefronts, tf_args.h TF_L1_SPLIT_MODEL) */
int tf_solver_kernel_block(tf_solver*, int32_t kernel, int32_t* block);
int tf_sync(tf_solver*);            /* waits for the stream, reports device-side failures */

/* ---- measurement: kernel begin/end timestamps (HIP events attached to the
 * launch) per kernel; mask bit k selects kernel k, -1 = all, 0 = off ---------- */
int tf_timing_enable(tf_solver*, int64_t mask);
int tf_timing_reset(tf_solver*);
int tf_timing_get(tf_solver*, int32_t kernel, double* total_ms, int64_t* launches);
/* diagnostic kernel builds (-DTF_STAMPS): shader-clock stamps of one workgroup per solver
 * level, out[level][64]; the first call only switches the recording on */
int tf_debug_stamps(tf_solver*, uint64_t* out, int32_t max_levels);
int tf_kernel_count(void);
const char* tf_kernel_name(int32_t kernel);

/* ---- device probes: per-step reductions of model expressions on a resident state slot ----------
 * code_object: the model's generated source with the generated probe block and csrc/tf_probe.h
 * (codegen.lower_probes; built with the solver's parameter layout and sweep segment): it holds
 * tfk_probe_partial / tfk_probe_final.  kinds[nprobe]: 0 sum, 1 mean, 2 integral
 * (np.trapz; periodic: dx * sum), 3 max, 4 min, 5 argmax, 6 argmin (x of the first extremal node);
 * NaN as numpy has it.  nconst: host constants of the probe expressions (codegen spec
 * "host_consts"), set per system by tf_probe_set_consts.  A record is queued on the solver's
 * stream (no host wait) and writes one row [nsys][nprobe] into a device ring of `capacity` rows,
 * which the host counts; a record that finds the ring full first copies it to host memory (one wait
 * per `capacity` records).  A probe belongs to its solver: destroy it first. */
typedef struct tf_probe tf_probe;
int tf_probe_create(tf_solver*, const void* code_object, size_t code_size, int32_t nprobe,
                    const int32_t* kinds, int32_t nconst, int32_t capacity, tf_probe** out);
void tf_probe_destroy(tf_probe* probe);
int tf_probe_set_consts(tf_probe*, const double* values /*[nsys][nconst]*/, int32_t nconst);
/* coordinates of the nodes (argmax / argmin, probes that read x); ignored when the solver's model reads
 * x itself: the probes then read the solver's plane (tf_set_x) */
int tf_probe_set_x(tf_probe*, const double* x /*[nsys][N]*/);
int tf_probe_record(tf_probe*, int32_t slot);
/* waits, then hands over the oldest rows recorded since the last fetch (at most max_rows of them,
 * out[row][nsys][nprobe]); *rows = how many */
int tf_probe_fetch(tf_probe*, double* out, int64_t max_rows, int64_t* rows);
/* rows recorded and not fetched yet (no wait) */
int tf_probe_pending(tf_probe*, int64_t* rows);

/* ---- device recorders: decimated space-time series of model expressions on a resident state slot ----
 * code_object: the model's generated source with the generated record block and csrc/tf_record.h
 * (codegen.lower_records; built with the solver's parameter layout and sweep segment): it holds tfk_record.
 * geometry[nrec][6]: the expression of the block (recorders may share one), pool (0 sample, 1 max,
 * 2 min, 3 mean), start, stop, step of the window of nodes (0 <= start < stop <= N, step >= 1) and
 * the rows of the recorder's device ring (>= 2: two halves).
 * Column j of a recorder is its expression pooled over nodes start + j*step ...
 * min(start + (j+1)*step, stop) - 1; NaN as numpy has it; the mean's sum is added in a fixed order.
 * A record is queued on the solver's stream (no host wait) and writes one row [nsys][ncols], which the
 * host counts; a half
 * of the ring that is full is copied to page-locked host memory by a stream of the recorder's own
 * while the records go on into the other half.  A recorder belongs to its solver: destroy it first. */
typedef struct tf_record tf_record;
int tf_record_create(tf_solver*, const void* code_object, size_t code_size, int32_t nrec,
                     const int32_t* geometry, int32_t nconst, tf_record** out);
void tf_record_destroy(tf_record* record);
int tf_record_set_consts(tf_record*, const double* values /*[nsys][nconst]*/, int32_t nconst);
/* coordinates of the nodes (expressions that read x); ignored when the solver's model reads x itself */
int tf_record_set_x(tf_record*, const double* x /*[nsys][N]*/);
int tf_record_record(tf_record*, int32_t which, int32_t slot);
/* waits, then hands over the oldest rows of recorder `which` recorded since its last fetch (at most
 * max_rows of them, out[row][nsys][ncols]); *rows = how many */
int tf_record_fetch(tf_record*, int32_t which, double* out, int64_t max_rows, int64_t* rows);
/* rows of recorder `which` recorded and not fetched yet (no wait) */
int tf_record_pending(tf_record*, int32_t which, int64_t* rows);

/* ---- device statistics: per-node statistics over time of model expressions on a resident state slot ----
 * code_object: the model's generated source with the generated statistic block and csrc/tf_stat.h
 * (codegen.lower_statistics; built with the solver's parameter layout and sweep segment): it holds
 * tfk_stat.  geometry[nstat][2]: the expression of the block (statistics may share one; the
 * expressions are numbered in the order the statistics first use them: 0, then at most one more) and
 * the kind: 0 mean, 1 var (running mean and sum of squared deviations M2; the variance is M2 / n),
 * 2 max, 3 min (NaN as numpy has it), 4 argmax, 5 argmin (the extremum and the t of the first sample
 * that attained it; the first NaN's t wins and stays).  A statistic owns one plane (mean, max, min) or
 * two (var: mean, M2; argmax, argmin: value, t) of [nsys][N] doubles.  An update is queued on the
 * solver's stream (no host wait) and folds state `slot` into statistic `which` as sample k (1, 2, ...;
 * the caller counts: sample 1 overwrites, so starting over costs nothing) taken at time t.  A statistic
 * set belongs to its solver: destroy it first. */
typedef struct tf_stat tf_stat;
int tf_stat_create(tf_solver*, const void* code_object, size_t code_size, int32_t nstat,
                   const int32_t* geometry, int32_t nconst, tf_stat** out);
void tf_stat_destroy(tf_stat* stat);
int tf_stat_set_consts(tf_stat*, const double* values /*[nsys][nconst]*/, int32_t nconst);
/* coordinates of the nodes (expressions that read x); ignored when the solver's model reads x itself */
int tf_stat_set_x(tf_stat*, const double* x /*[nsys][N]*/);
int tf_stat_update(tf_stat*, int32_t which, int32_t slot, int64_t k, double t);
/* planes of statistic `which` (1 or 2, by its kind): the size of what fetch hands over and load takes */
int tf_stat_planes_of(tf_stat*, int32_t which, int32_t* planes);
/* waits, then hands over the planes of statistic `which` in natural order, out[planes][nsys][N] */
int tf_stat_fetch(tf_stat*, int32_t which, double* out);
/* the inverse of tf_stat_fetch: in[planes][nsys][N] become the planes of statistic `which` */
int tf_stat_load(tf_stat*, int32_t which, const double* in);

/* ---- device spectra: Fourier amplitudes of model expressions on a resident state slot ----
 * code_object: the model's generated source with the generated spectrum block and csrc/tf_spectrum.h
 * (codegen.lower_spectra; built with the solver's parameter layout and sweep segment): it holds
 * tfk_spectrum_partial and tfk_spectrum_final.  geometry[nspec][3]: the expression of the block (spectra may share
 * one; the expressions are numbered in the order the spectra first use them), the number of modes
 * (1 ... 64) and the rows of the spectrum's ring in device memory.  The modes themselves (each 0 ... N/2)
 * are data of the handle: set_modes before the first record.  A record is queued on the solver's stream
 * (no host wait unless the ring is full: then all of it comes over in one copy first) and writes one row
 * [nsys][nmodes] of (re, im) pairs, c = sum over the nodes g of v_g exp(-2 pi i m g / N).  A spectrum
 * set belongs to its solver: destroy it first. */
typedef struct tf_spectrum tf_spectrum;
int tf_spectrum_create(tf_solver*, const void* code_object, size_t code_size, int32_t nspec,
                       const int32_t* geometry, int32_t nconst, tf_spectrum** out);
void tf_spectrum_destroy(tf_spectrum* spectrum);
int tf_spectrum_set_consts(tf_spectrum*, const double* values /*[nsys][nconst]*/, int32_t nconst);
/* coordinates of the nodes (expressions that read x); ignored when the solver's model reads x itself */
int tf_spectrum_set_x(tf_spectrum*, const double* x /*[nsys][N]*/);
int tf_spectrum_set_modes(tf_spectrum*, int32_t which, const int32_t* modes, int32_t nmodes);
int tf_spectrum_record(tf_spectrum*, int32_t which, int32_t slot);
/* waits, then hands over up to max_rows rows of spectrum `which` not fetched before, oldest first,
 * out[rows][nsys][nmodes][2] */
int tf_spectrum_fetch(tf_spectrum*, int32_t which, double* out, int64_t max_rows, int64_t* rows);
/* rows of spectrum `which` recorded and not fetched yet (no wait) */
int tf_spectrum_pending(tf_spectrum*, int32_t which, int64_t* rows);

/* ---- device extrema: crests and troughs of model expressions on a resident state slot ----
 * code_object: the model's generated source with the generated extrema block and csrc/tf_extrema.h
 * (codegen.lower_extrema; built with the solver's parameter layout and sweep segment): it holds
 * tfk_extrema_count and tfk_extrema_write.  geometry[next][4]: the expression of the block (observers may share
 * one; the expressions are numbered in the order the observers first use them), the kind (0: max, 1: min),
 * max_count (1 ... 8192) and the rows of the observer's ring in device memory (0: 1024 rows, or what 32 MB
 * hold; a single row that is larger is refused).  thresholds[next]: a maximum counts when it is greater, a
 * minimum when it is less (-inf / +inf: none).  Node g is a maximum iff v[g-1] < v[g] > v[g+1], strictly,
 * and v[g] is finite; the neighbours wrap on a periodic grid, the end nodes of any other are never extrema.
 * A record is queued on the solver's stream (no host wait unless the ring is full: then all of it comes
 * over in one copy first) and writes one row [nsys][1 + 4 * max_count]: the number of extrema of the system
 * (it may exceed max_count), then the first max_count of them in node order as (g, v[g-1], v[g], v[g+1]);
 * the entries past the count are not written.  An extrema set belongs to its solver: destroy it first. */
typedef struct tf_extrema tf_extrema;
int tf_extrema_create(tf_solver*, const void* code_object, size_t code_size, int32_t next,
                      const int32_t* geometry, const double* thresholds, int32_t nconst, tf_extrema** out);
void tf_extrema_destroy(tf_extrema* extrema);
int tf_extrema_set_consts(tf_extrema*, const double* values /*[nsys][nconst]*/, int32_t nconst);
/* coordinates of the nodes (expressions that read x); ignored when the solver's model reads x itself */
int tf_extrema_set_x(tf_extrema*, const double* x /*[nsys][N]*/);
int tf_extrema_record(tf_extrema*, int32_t which, int32_t slot);
/* waits, then hands over up to max_rows rows of observer `which` not fetched before, oldest first,
 * out[rows][nsys][1 + 4 * max_count] */
int tf_extrema_fetch(tf_extrema*, int32_t which, double* out, int64_t max_rows, int64_t* rows);
/* rows of observer `which` recorded and not fetched yet (no wait) */
int tf_extrema_pending(tf_extrema*, int32_t which, int64_t* rows);

/* ---- device histograms: value distributions of model expressions on a resident state slot ----
 * code_object: the model's generated source with the generated histogram block and csrc/tf_histogram.h
 * (codegen.lower_histograms; built with the solver's parameter layout and sweep segment).  It
 * holds tfk_hist_partial and tfk_hist_final: they are not in the kernel table (tf_kernel_name), are
 * resolved by name here and are not covered by tf_timing_get.  geometry[nhist][6]: the expression of the
 * block (histograms may share one; the expressions are numbered in the order the histograms first use
 * them), the number of bins (1 ... 256), the rows of the histogram's ring in device memory and the window
 * of nodes (start, stop, step: slice.indices(N), step >= 1).  The nbins + 1 edges (finite, strictly
 * increasing) are data of the handle: set_edges before the first record.  A record is queued on the
 * solver's stream (no host wait unless the ring is full: then all of it comes over in one copy first) and
 * writes one row [nsys][nbins + 3] of counts as doubles: bin i counts edges[i] <= v < edges[i + 1] over the
 * window nodes, the last bin also v == edges[nbins]; then v < edges[0], v > edges[nbins] and the NaNs.  A
 * histogram set belongs to its solver: destroy it first. */
typedef struct tf_histogram tf_histogram;
int tf_histogram_create(tf_solver*, const void* code_object, size_t code_size, int32_t nhist,
                        const int32_t* geometry, int32_t nconst, tf_histogram** out);
void tf_histogram_destroy(tf_histogram* histogram);
int tf_histogram_set_consts(tf_histogram*, const double* values /*[nsys][nconst]*/, int32_t nconst);
/* coordinates of the nodes (expressions that read x); ignored when the solver's model reads x itself */
int tf_histogram_set_x(tf_histogram*, const double* x /*[nsys][N]*/);
int tf_histogram_set_edges(tf_histogram*, int32_t which, const double* edges, int32_t nedges);
int tf_histogram_record(tf_histogram*, int32_t which, int32_t slot);
/* waits, then hands over up to max_rows rows of histogram `which` not fetched before, oldest first,
 * out[rows][nsys][nbins + 3] */
int tf_histogram_fetch(tf_histogram*, int32_t which, double* out, int64_t max_rows, int64_t* rows);
/* rows of histogram `which` recorded and not fetched yet (no wait) */
int tf_histogram_pending(tf_histogram*, int32_t which, int64_t* rows);

/* ---- device hooks: a program of statements that WRITES a resident state from model expressions ----
 * What the reference does with hook(t, fields, pars) on the host -- boundary values tied to other nodes or
 * fields, an outflow copy, a sponge layer, a positivity clip -- done by two kernels on the state where it
 * lives.  The contract is the Python function that executes the statements in the order given:
 *
 *     for (var, target, expression) in statements:  fields[var][target] = value(expression)
 *
 * with the right-hand side evaluated completely before the assignment (NumPy's rule) and every statement
 * seeing the assignments of the statements before it.  A point statement has a node as its target; the
 * names of its expression are the fields at that node, and at(name, k) is field `name` at the absolute
 * node k.  A window statement has the nodes start, start + step, ... < stop; the names are the fields at
 * the node being assigned (no at(), no stencil: the program assigns in place).  x is the coordinate of the
 * node, t the time of the call.  A value is the bits NumPy computes from the printed expression
 * (codegen.lower_hooks: same emitter as F).
 *
 * code_object: the model's generated source with the generated hook block and csrc/tf_hook.h, built with
 * the solver's parameter layout and sweep segment.  It holds tfk_hook_window and tfk_hook_points: they are
 * not in the kernel table (tf_kernel_name), are resolved by name here and are not covered by
 * tf_timing_get.  geometry[nstatement][5]: kind (0 point, 1 window), the index of the target variable and
 * the target (node, 0, 0 or start, stop, step = slice.indices(N), step >= 1; an empty window is legal) --
 * what the static tables of the block hold, here for the runtime to check against the grid and to size
 * its launches by: one launch per maximal run of consecutive statements of one kind, a run of window
 * statements over the chunks and rows the union of its windows touches and no others.
 *
 * set_consts: the host constants of the expressions ([nsys][nconst]; powers and libm calls of uniform
 * arguments, t among them, evaluated by NumPy on the host) for the call before the step and for the call
 * after it, with the two times.  They live in device memory and nothing of t is a launch argument: upload
 * them between the steps (never inside one) and a step replayed from a captured graph sees them.
 * attach: while on, the step functions apply the program wherever they apply the Dirichlet list, after
 * it -- to the copy of the input with the `before` set, to the result with the `after` set.  idempotent
 * != 0 says that no right-hand side reads a field, so an input that a step of this solver left with the
 * same values applied is read in place (as with the Dirichlet list); any other program is applied to a
 * copy of the input every time.  One program is attached to a solver at a time; attach(0) before the
 * handle or another program's attach.  apply: one application outside a step with the `before` set, slot
 * src -> slot dst (src == dst: in place).  A hook belongs to its solver: detach and destroy it first. */
typedef struct tf_hook tf_hook;
int tf_hook_create(tf_solver*, const void* code_object, size_t code_size, int32_t nstatement,
                   const int32_t* geometry, int32_t nconst, tf_hook** out);
void tf_hook_destroy(tf_hook* hook);
/* coordinates of the nodes (expressions that read x); ignored when the solver's model reads x itself */
int tf_hook_set_x(tf_hook*, const double* x /*[nsys][N]*/);
int tf_hook_set_consts(tf_hook*, const double* before /*[nsys][nconst]*/, const double* after /*[nsys][nconst]*/,
                       double t_before, double t_after);
int tf_hook_attach(tf_hook*, int32_t on, int32_t idempotent);
int tf_hook_apply(tf_hook*, int32_t src, int32_t dst);

#ifdef __cplusplus
}
#endif
#endif
