/*
 * mfgp_hip.h -- C ABI of the MI355X GP posterior engine (libmfgp_hip.so).
 *
 * Drop-in boundary for the hot path of MSU-dcypherlab/mfgp-coverage: the
 * reference has no FFI layer, its boundary is the Python class API of
 * gaussian_process.py (imported at simulator.py:25). Each entry point below
 * replaces one reference method; the Python mirror
 * (mfgp_coverage_amd/gaussian_process.py) binds them with ctypes
 * (see INTEGRATION.md).
 *
 * Conventions
 *   - plain pointers and sizes; no torch / HIP types in the signatures
 *     (streams are passed as void*, i.e. a hipStream_t).
 *   - coordinates are row-major [n,2] float64, values [n] float64.
 *   - every data pointer may be host or device memory (detected with
 *     hipPointerGetAttributes); inputs are borrowed for the call and copied,
 *     outputs are written into caller buffers.
 *   - return 0 on success, else an MFGP_ERR_* code; mfgp_last_error() gives a
 *     thread-local message.
 */
#ifndef MFGP_HIP_H
#define MFGP_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MFGP_OK 0
#define MFGP_ERR_NOT_PD 1   /* Cholesky pivot <= 0: numpy.linalg.LinAlgError (gp:254, gp:529) */
#define MFGP_ERR_ARG 2      /* bad argument: TypeError/ValueError (simulator.py:366, 652)     */
#define MFGP_ERR_DEVICE 3   /* HIP runtime error: RuntimeError                                */
#define MFGP_ERR_NO_V 4     /* mfgp_cov_block: the resident V does not cover the model's rows   */
#define MFGP_ERR_NO_LATTICE 5   /* the grid is not a lattice, or a training row is not one of its cells */

#define MFGP_SF 0           /* SFGP, gaussian_process.py:23-268, hyp [mu, s2, L, noise]              */
#define MFGP_MF 1           /* MFGP, gaussian_process.py:271-578, hyp [mu_lo,s2_lo,L_lo,mu_hi,s2_hi,
                               L_hi,rho,noise_lo,noise_hi] (all log-scaled, simulator.py:53-56)     */
#define MFGP_F64 0
#define MFGP_F32 1          /* BASELINE configs[4]: the resident V = L^-1 psi^T stored and streamed
                               in fp32, and the lattice step's F = L^-1 streamed in fp32 (built in
                               fp64, rounded once per build); factor, solves and reductions fp64.
                               Tolerance vs the fp64 oracle: oracle/gp_oracle.py parity_errors_f32
                               (F32_TOL = 1e-4) */

#define MFGP_ASYNC 1        /* batch flag: do not synchronise; status via mfgp_ctx_synchronize */

typedef struct mfgp_ctx mfgp_ctx;
typedef struct mfgp_model mfgp_model;

/* One context per host thread: owns a HIP stream and a scratch workspace. */
int mfgp_ctx_create(int device, mfgp_ctx** out);
void mfgp_ctx_destroy(mfgp_ctx* ctx);
/* Give back the context's scratch (the fp64 V scratch of MFGP_F32 full predicts,
 * up to 16 GB, and the workspace) after synchronising; the next call that needs
 * it allocates it again. Models keep their resident state. */
int mfgp_ctx_trim(mfgp_ctx* ctx);
/* Members per set of launches for mfgp_nlml_batch: 0 = automatic (default: as many as
 * 4 GiB of scratch hold, at most 256); a larger value is taken as 256. The results do
 * not depend on it. Its scratch is given back by mfgp_ctx_trim as well. */
int mfgp_ctx_set_nlml_chunk(mfgp_ctx* ctx, int max_members);
/* Launch on a caller stream (hipStream_t) instead of the context's own. NULL restores it. */
int mfgp_ctx_set_stream(mfgp_ctx* ctx, void* hip_stream);
void* mfgp_ctx_get_stream(mfgp_ctx* ctx);
/* Wait for all work; returns MFGP_ERR_NOT_PD if an ASYNC batch hit a non-PD factor. */
int mfgp_ctx_synchronize(mfgp_ctx* ctx);
/* Incremental updates (default on): an append of k <= 16 rows to a current
 * factor is a bordered Cholesky step (L21 = K21 L11^-T, L22 = chol(K22 - L21 L21^T))
 * instead of the reference's full refactor (gp:254 / gp:529), and predict keeps
 * V = L^-1 psi^T resident so that it streams V once instead of recomputing it.
 * Results agree with the full path to rounding. 0 = refactor and recompute V
 * on every update, as the reference does. */
int mfgp_ctx_set_incremental(mfgp_ctx* ctx, int enable);
/* With incremental updates: run a batch's bordered appends and the one-pass
 * predicts that follow them as ONE launch (k_inc_stream: the append's producer
 * workgroups hand L21 / L22 to the cell tiles inside the kernel). Default on;
 * 0 = two launches (k_inc_stream for the append alone, then k_vstream). Same
 * numbers either way. */
int mfgp_ctx_set_fused(mfgp_ctx* ctx, int enable);
/* Deferred appends (default 0): mfgp_append of rows that a bordered append can
 * take only stages them; the next call that needs the factor runs the append --
 * mfgp_predict as one launch with the one-pass predict (the single-model form of
 * the batched path). A non-positive-definite append is then reported by that
 * call instead of by mfgp_append (the reference raises in updt / updt_hifi,
 * gp:254 / gp:529). */
int mfgp_ctx_set_deferred_appends(mfgp_ctx* ctx, int enable);
/* Lattice-separable appends (default on): when the grid is a lattice, kss /
 * (smallest noise + jitter) <= 1e4 and the model holds the posterior of the old
 * rows, a bordered append + predict of k <= 16 rows runs as k_inc_lat: w =
 * K11^-1 K12 from the resident explicit inverse L^-1, then the SE kernel's
 * separability over the two lattice axes turns L21 V_old into Z rows (per lattice
 * y-row, the sum of w c ex over the training rows on it) times axis-table rows,
 * a GEMM over 2 ny terms (f64 MFMA; a training row off the lattice adds one term)
 * -- no pass over V -- and var / mu are updated from the previous posterior.
 * Batches whose V stream is estimated cheaper (one GP at the headline size) keep
 * it; 2 = take the lattice step for them too (tests). 0 = always the V stream
 * (k_inc_stream). Same numbers to rounding. */
int mfgp_ctx_set_lattice(mfgp_ctx* ctx, int enable);
/* The column store of V in the lattice step. A model in the lattice mode also keeps V
 * by columns (Vc[cell][row], the memory of V again, within mfgp_ctx_set_vcol_budget):
 * the step's producers and w units then read a new point's L21 row as contiguous
 * bytes, and the w units start their pass over F at launch instead of after the
 * producers' compact rows. mode -1 (default): a batch whose models all have a store
 * takes it; 0: never, and no store is allocated; 1: as -1. Same bits either way.
 * Also the environment variable MFGP_LAT_VCOL (0 / 1 / auto) at mfgp_ctx_create. */
int mfgp_ctx_set_lattice_vcol(mfgp_ctx* ctx, int mode);
/* Bytes one model's column store may take (-1: the built-in bound, 1 GiB, and a
 * quarter of the free device memory; 0: no model gets a store). Models that have one
 * keep it until their grid or row capacity changes. */
int mfgp_ctx_set_vcol_budget(mfgp_ctx* ctx, int64_t bytes);
/* Declare that this context's launches may run concurrently with launches of
 * other contexts on the same GPU (several streams stepping independent batches
 * side by side, e.g. a rank's seeds as four sub-batches). Default 0. With it no
 * launch relies on all of its workgroups being resident at once: the lattice
 * step always runs its GEMM as the second launch (k_lat_gemm2) rather than as
 * split-K tiles that wait for each other inside the first. Every other
 * cross-workgroup wait in the library is on a workgroup with a lower linear id,
 * dispatched (and so resident) before its waiter, which stays safe when other
 * kernels share the GPU. */
int mfgp_ctx_set_concurrent(mfgp_ctx* ctx, int enable);
/* Kernel timing with HIP events on the launch stream: enable = 1 times every
 * predict-kernel launch (fused predict or one-pass incremental predict) and
 * every factor stage; 2 times the predict launches only (each event pair is a
 * few microseconds of stream time); 0 = off. */
int mfgp_ctx_enable_timing(mfgp_ctx* ctx, int enable);
/* Bracket only every stride-th eligible launch with events (default 1), so a
 * timed run samples kernel durations without paying the events on every step. */
int mfgp_ctx_set_timing_stride(mfgp_ctx* ctx, int64_t stride);
/* Sum of predict-kernel durations (ms) and launch count since the last reset;
 * also the same for the factor stage (assemble + blocked Cholesky). */
int mfgp_ctx_get_timing(mfgp_ctx* ctx, double* predict_ms, int64_t* predict_launches,
                        double* factor_ms, int64_t* factor_calls);
int mfgp_ctx_reset_timing(mfgp_ctx* ctx);
/* Path counters of the planners' loops (mfgp_sample_points,
 * mfgp_batch_sample_points: each model's appended rows, dropped at the end) since
 * the last reset: out[0..n) = {model runs, bordered appends, one-pass predicts (V stream or
 * lattice step), lattice steps, of them launched with their descriptors by
 * value, of them with the GEMM and cells as a second launch, full refactors, full
 * predicts, then the batched planner's host time in microseconds before, in and
 * after its iteration loop}; n <= 11. reset != 0 zeroes them after the read. Which
 * step form the Choi iterations took and where their time went (tools/bench_planner.py). */
int mfgp_ctx_planner_stats(mfgp_ctx* ctx, int64_t* out, int n, int reset);

/* SFGP.__init__ (gp:28-64) / MFGP.__init__ (gp:276-327) with the caller's
 * hyperparameters (the simulator overwrites .hyp right after construction,
 * simulator.py:72-73, 99-100). nhyp = 4 (SF) or 9 (MF). jitter = 1e-8 in the
 * reference (gp:42, gp:298). */
int mfgp_model_create(mfgp_ctx* ctx, int kind, int dtype, const double* hyp, int nhyp,
                      double jitter, mfgp_model** out);
void mfgp_model_destroy(mfgp_model* m);
/* copy.deepcopy(model) (simulator.py:339). */
int mfgp_clone(const mfgp_model* src, mfgp_model** out);
/* Writes to .hyp / .jitter; they take effect at the next factorisation. */
int mfgp_model_set_hyp(mfgp_model* m, const double* hyp, int nhyp, double jitter);

/* The grid X* of predict(X_star) (gp:121 / gp:401), [M,2]. Cached on the device. */
int mfgp_set_grid(mfgp_model* m, const double* xstar, int64_t M);

/* updt_info (gp:229-255 / gp:493-529): replace the training set and refactor.
 * SF uses only the H slots (XL/yL must be NULL/0). Returns MFGP_ERR_NOT_PD like
 * np.linalg.cholesky raising LinAlgError. */
int mfgp_set_data(mfgp_model* m, const double* XL, const double* yL, int64_t NL,
                  const double* XH, const double* yH, int64_t NH);

/* updt (gp:257-268) / updt_hifi (gp:531-542): append k >= 0 rows and refactor.
 * When the previous append was followed by a predict (the simulator's step), the
 * append also runs the one-pass predict in the same launch and keeps the result
 * for the next mfgp_predict; a non-PD step is still reported here. That launch
 * publishes the step's positive-definiteness verdict as soon as it has it, and
 * mfgp_append returns then, while the launch computes the posterior: the next
 * entry point called on the context waits for the launch first (and reports a
 * failure of its later phases, e.g. a hand-off wait's timeout), so the caller's
 * host work in between overlaps it (MFGP_EARLY_PD=0: return at the launch's end). */
int mfgp_append(mfgp_model* m, const double* X, const double* y, int64_t k);

/* predict (gp:121-148 / gp:401-438): posterior mean and the diagonal of the
 * posterior covariance at every grid cell (the only part the callers use,
 * simulator.py:301, 341, 672, 685, 842, 855, 1014). mu, var: [M], host or
 * device memory. Results for host buffers are kept with the model: predicts of
 * an unchanged model return them again (the same bits, no launch). */
int mfgp_predict(mfgp_model* m, double* mu, double* var);
/* mfgp_predict without the host copy (the drop-in predict's path): the result is
 * left in the model's mapped pinned result buffer, which is handed over to the
 * caller -- *mu, *var point into it (writable, [M] each) until
 * mfgp_release_view(*view); the model takes another buffer from a process-wide
 * pool for its next host-bound predict, so a predict of an unchanged model after
 * a view recomputes. M = 0: *mu = *var = *view = NULL. */
int mfgp_predict_view(mfgp_model* m, double** mu, double** var, void** view);
/* mfgp_predict_view that may hand over the buffer of an eager append's launch
 * still computing into it (mfgp_append above): then *running = 1 and the caller
 * must call mfgp_ctx_synchronize before it reads the buffer or gives it to anyone
 * (the drop-in predict wraps the arrays meanwhile); else *running = 0 and it is
 * mfgp_predict_view. */
int mfgp_predict_view_running(mfgp_model* m, double** mu, double** var, void** view, int* running);
/* Return a buffer handed over by mfgp_predict_view (any thread, any time, also
 * after its model or context is destroyed). */
int mfgp_release_view(void* view);
/* The fused np.amax / np.argmax of a handed-over buffer's variance (the eager
 * append's launch reduces them beside its status word): *valid = 1 and the max
 * and its first cell when the launch that wrote the buffer computed them, else
 * *valid = 0 (a predict without an append before it). Read after the buffer is
 * ready (mfgp_predict_view_running: after mfgp_ctx_synchronize). */
int mfgp_view_max(const void* view, double* vmax, int64_t* argmax, int* valid);

/* A block of the dense posterior covariance that predict returns in the
 * reference (gp:146 / gp:435-436): out[i * ldo + j] = cov(x_rows[i], x_cols[j]) =
 * k**(x_i, x_j) - sum_n V[n, i] V[n, j] over the model's N training rows, from the
 * resident V = L^-1 psi^T (k_cov_block: one f64-MFMA GEMM over V's rows plus the
 * prior term; no M x M intermediate). rows / cols: host arrays of grid cell
 * indices in [0, M), in any order, repeats allowed; NULL = all cells 0..M-1 (then
 * na / nb must equal M). out: host or device memory, row-major with leading
 * dimension ldo >= nb. flags: MFGP_COV_PRIOR = the prior covariance k** alone (no
 * factor needed). The call first brings the model to the state mfgp_predict leaves
 * (a pending or deferred append, new hyperparameters or a new grid run their
 * factor and predict here, and MFGP_ERR_NOT_PD surfaces as there); if V still
 * does not cover the N rows it returns MFGP_ERR_NO_V. Every index is validated
 * before anything is enqueued: an index outside [0, M), ldo < nb or a model
 * without a grid returns MFGP_ERR_ARG, launches nothing and leaves the model as
 * it was. na == 0 or nb == 0: MFGP_OK, nothing written. MFGP_F32 models:
 * MFGP_ERR_ARG (their fp32 V needs its own tolerance policy). An entry's bits
 * depend only on its pair of cells: block(a, b) == block(b, a)^T, any block
 * equals the same entries of the full matrix, and two calls agree bit for bit. */
#define MFGP_COV_PRIOR 1
int mfgp_cov_block(mfgp_model* m, const int64_t* rows, int64_t na, const int64_t* cols, int64_t nb,
                   double* out, int64_t ldo, int flags);
/* Integrated variance reduction per candidate cell (the A-optimal criterion): how
 * much the weighted posterior variance of the whole grid falls if the hifi field is
 * measured at grid cell cand[j],
 *   out[k * ldo + j] = sum_i w[k * ldw + i] cov(i, cand[j])^2 / (cov(cand[j], cand[j]) + noise_H + jitter),
 * i over all M cells (noise_H + jitter: the diagonal term a hifi append adds to K; an
 * SF model's single noise), from the resident V (k_ivr_partial: k_cov_block's GEMM
 * with the column sums of w o cov^2 reduced in registers, so the M x nc block never
 * exists; k_ivr_finish: the division and the maxima). cand: a host array of grid cell
 * indices in [0, M), any order, repeats allowed; NULL = all cells (then nc must equal
 * M). w: nw <= MFGP_IVR_MAXW weight vectors [nw][ldw], ldw >= M, host or device
 * memory; NULL = one vector of ones (then nw must be 1). Row tiles of 64 cells whose
 * weights are zero in every vector are skipped, so a region mask costs its region.
 * out: [nw][ldo], ldo >= nc, host or device memory. best / best_pos: host [nw], each
 * optional: the maximum of out's row k and its first position in the candidate list.
 * The call settles the model as mfgp_cov_block does (MFGP_ERR_NOT_PD, MFGP_ERR_NO_V as
 * there) and validates everything before anything is enqueued: an index out of range,
 * nw outside [1, MFGP_IVR_MAXW], ldw < M, ldo < nc, a non-finite weight in a host
 * buffer, a model without a grid and an MFGP_F32 model return MFGP_ERR_ARG, launch
 * nothing and leave the model as it was. nc == 0: MFGP_OK, nothing written. A model
 * without training rows gives the prior's score (a grid, no factor needed). The model
 * itself is not changed. out[k][j] depends bit for bit only on the model, the cell
 * cand[j] and the weight vector k -- not on nc, j, the other candidates, nw or the
 * other vectors -- and two calls agree bit for bit. */
#define MFGP_IVR_MAXW 8
int mfgp_var_reduction(mfgp_model* m, const int64_t* cand, int64_t nc, const double* w, int nw, int64_t ldw,
                       double* out, int64_t ldo, double* best, int64_t* best_pos);
/* The posterior covariance applied to grid vectors,
 *   out[k * ldo + i] = sum_j cov(i, j) x[k * ldx + j],   i, j over all M cells, k < nx,
 * for nx <= MFGP_IVR_MAXW vectors, from the resident V: cov x = K** x - V^T (V x), two
 * streamed passes over V per vector (k_cov_dot, k_cov_apply) and the prior's product, so
 * the M x M matrix never exists -- the one covariance quantity a grid too large for
 * mfgp_cov_block's dense block still gives (w^T cov w: the variance of the field's mass
 * over a region). K** x: on a lattice grid with axes of at most 256 values the kernel
 * factorises over the axes and the product is two small matrix products per kernel
 * part; on any other grid k** is evaluated entry by entry (M^2 exponentials: meant for
 * grids of a few thousand cells). The two forms agree to rounding, not bit for bit;
 * the environment variable MFGP_PLAN_SEP=0 (read at mfgp_ctx_create) forces the second.
 * x: [nx][ldx], ldx >= M; out: [nx][ldo], ldo >= M; each host or device memory.
 * flags: MFGP_COV_PRIOR = K** x alone (no factor needed); a model without training
 * rows gives the same. The call settles the model as mfgp_cov_block does
 * (MFGP_ERR_NOT_PD, MFGP_ERR_NO_V as there) and validates everything before anything
 * is enqueued: a model without a grid, an MFGP_F32 model, nx outside
 * [1, MFGP_IVR_MAXW], ldx < M, ldo < M, a null pointer and a non-finite value in a host
 * x return MFGP_ERR_ARG, launch nothing and leave the model as it was. The model
 * itself is not changed (serial, counters, V and posterior stay). The vectors run one
 * after another: out's row k depends bit for bit only on the model and x's row k -- not
 * on nx, k or the other rows -- and two calls agree bit for bit. */
int mfgp_cov_apply(mfgp_model* m, const double* x, int nx, int64_t ldx, double* out, int64_t ldo, int flags);
/* The model's posterior serial: a value that changes whenever its training rows,
 * hyperparameters, jitter or grid change (appends, the batch entry points,
 * mfgp_truncate, mfgp_set_data / _set_hyp / _set_grid, the planners' loops), and is
 * never reused within the process -- truncate followed by an append of the same
 * count gives a new one. What a holder of an earlier result compares to know
 * whether the model still holds that posterior. No device work. */
int mfgp_model_serial(const mfgp_model* m, uint64_t* serial);

/* The posterior at arbitrary points, optionally conditioned on prospective points
 * that are not in the model (MFGP.pred_var, gp:440-481; get_neg_var, gp:544-563):
 * Xq [nq,2] query points (hifi targets, as in predict); XL_new [nl_new,2] /
 * XH_new [nh_new,2] prospective lofi / hifi rows, at most MFGP_LOOK_MAX together
 * (an SF model takes its rows in XH_new; nl_new must be 0). Prospective rows carry
 * no values: they change the variance, not the mean. Outputs, each or NULL:
 *   mu [nq]    posterior mean of the current model
 *   var0 [nq]  posterior variance of the current model
 *   var [nq]   variance with the prospective rows added (== var0 without any)
 *   cov [nq, ldc] row-major, ldc >= nq: the dense look-ahead covariance
 * Pointers are host or device memory. Every argument is checked before anything
 * is enqueued (counts, ldc, finite coordinates: MFGP_ERR_ARG). The call settles a
 * running launch and brings the factor up to date as mfgp_get_factor does (pending
 * or deferred appends, new hyperparameters); it needs no grid. Of the model it
 * changes nothing else but its look-ahead record and the two counters of
 * mfgp_model_stats: rows, serial, grid, resident V and posterior, kept predict
 * results and the path counters stay, so a predict before and after returns the
 * same bits by the same path. The border of a prospective set (k_look_border) is
 * kept in the record, keyed by the model's serial and the set's bytes and
 * fidelities: a repeated call with the same set on an unchanged model runs
 * k_look_query only. The record is allocated at the first call, freed with the
 * model and not copied by mfgp_clone. A border that is not positive definite
 * returns MFGP_ERR_NOT_PD (np.linalg.cholesky raising inside pred_var). A query's
 * mu / var0 / var bits depend on its own point only, not on its place in Xq or on
 * the other points. MFGP_F32 models are served in full fp64 (factor, Linv and z
 * are fp64; V is not involved). */
#define MFGP_LOOK_MAX 64   /* prospective points per call */
int mfgp_query(mfgp_model* m, const double* Xq, int64_t nq,
               const double* XL_new, int64_t nl_new, const double* XH_new, int64_t nh_new,
               double* mu, double* var0, double* var, double* cov, int64_t ldc);

/* Pathwise (Matheron) joint samples on the whole grid, at a cost linear in M: a prior
 * sample corrected through the data,
 *   f_post(grid) = m_H + f_prior(grid) + psi K^-1 (y - m - f_prior(X) - eps)
 *                = m_H + f_prior(grid) + V^T L^-1 r,
 *   r = (y - m) - f_prior(X) - sqrt(noise_fid + jitter) eps,
 * whose covariance is k** - psi K^-1 psi^T and whose mean is mfgp_predict's mu. The grid
 * must be a lattice and every training row one of its cells: the SE kernel separates
 * over the two axes, so sqrt(s) Ax Z Ay^T with Ax Ax^T = Kx, Ay Ay^T = Ky has the prior
 * covariance (an MF model: two independent fields u_L and delta, hifi = rho u_L + delta,
 * a lofi row sees u_L). The axis factors are diagonally pivoted Cholesky factors in fp64
 * on the host, of the unit-diagonal axis Gram exp(-(a_i / l - a_j / l)^2 / 2), stopped
 * when the largest remaining diagonal entry is <= 2^-50 (|A A^T - K| is bounded by that
 * plus rounding), stored n x rank. A sample takes nz = sum over fields rx ry + N normals. */
#define MFGP_SAMPLE_PRIOR 1     /* zero-mean draws of the hifi prior k** (no data, no factor needed) */

/* Host only, no device work: the pivoted-Cholesky factor of one axis. A is [n][n]
 * row-major, columns >= *rank zero. MFGP_ERR_ARG: a NULL pointer, n < 0, a length scale
 * that is not positive and finite, an axis value that is not finite. */
int mfgp_sample_axis_factor(const double* axis, int n, double lengthscale, double* A, int* rank);

/* dims[0..n): {nz, M, N, fields, rx0, ry0, rx1, ry1}; n <= 8. Settles the model as
 * mfgp_sample_posterior does (with MFGP_SAMPLE_PRIOR: nz without N, N = 0, nothing settled). */
int mfgp_sample_dims(mfgp_model* m, int64_t* dims, int n, int flags);

/* normals [S][ldz] (ldz >= nz): per sample field 0's rx0*ry0 block (row-major, x index
 * outer), field 1's, then one normal per training row in model order. out [S][ldo]
 * (ldo >= M), a sample's cells contiguous in grid order. Host or device pointers.
 * Every argument is checked before anything is enqueued: S < 0, ldz < nz, ldo < M, NULL
 * pointers with S > 0, non-finite normals in a host buffer, a model without a grid or an
 * MFGP_F32 model (as mfgp_cov_block) return MFGP_ERR_ARG, launch nothing and leave the
 * model as it was. S == 0: MFGP_OK, nothing written. The call first brings the model to
 * the state mfgp_predict leaves (a pending or deferred append, new hyperparameters or a
 * new grid are settled there, MFGP_ERR_NOT_PD surfaces as there); if V still does not
 * cover the N rows it returns MFGP_ERR_NO_V. A grid that is not a lattice, or a training
 * row that is no cell of it, returns MFGP_ERR_NO_LATTICE. flags: MFGP_SAMPLE_PRIOR = the
 * noise block of the normals is not read and nz excludes N; N = 0 without it gives
 * m_H + prior. Of the model the call changes only its sample record (the axis factors,
 * keyed by the model's serial, and the rows' lattice indices; allocated at the first
 * call, freed with the model, not cloned) and the counters sample_solve / sample_gemm of
 * mfgp_model_stats: rows, serial, grid, V, F and the lattice tables, the resident
 * posterior, the kept predict result and the path counters stay, so a predict before and
 * after returns the same bits by the same path. S > 64 runs in chunks of 64 (k_sample_t,
 * k_sample_field, k_sample_resid, k_sample_solve, k_sample_gemm per chunk). A sample's
 * bits depend only on its own nz normals: not on S, on its position, on the other
 * samples or on the chunking, and two calls agree bit for bit. */
int mfgp_sample_posterior(mfgp_model* m, const double* normals, int64_t S, int64_t ldz,
                          double* out, int64_t ldo, int flags);

/* Sizes and state readers (the Python mirror's .X/.L attributes). */
int64_t mfgp_model_n(const mfgp_model* m);      /* N = NL + NH */
int64_t mfgp_model_nl(const mfgp_model* m);
int64_t mfgp_model_m(const mfgp_model* m);
/* Path introspection (tests / benchmarks): out[0..n) = {factor rows (-1 = none),
 * resident V rows, full refactors, bordered appends, full predicts, one-pass
 * predicts (V stream or lattice step), grid lattice axes nx, ny (0 = the grid is
 * not a lattice: appends locate new points by a scan), lattice steps, off-lattice
 * training rows of the last lattice step (read back from the device; synchronises
 * the context's stream; only when n > 9), lattice steps launched with their
 * descriptors as the kernel argument, lattice steps whose GEMM and cells ran as a
 * second launch (k_lat_gemm2 or k_lat_gemm3), batch predicts served from the
 * resident posterior because the model appended nothing (k_post_copy), eager
 * appends of one GP that returned at the launch's published L22 verdict
 * (mfgp_append above), k_look_border launches and k_look_query launches of
 * mfgp_query (index 14 look_border, 15 look_query), k_sample_solve and k_sample_gemm
 * launches of mfgp_sample_posterior (index 16 sample_solve, 17 sample_gemm), lattice
 * steps whose w units read the column store of V (index 18 lattice_vcol; a step with a
 * new point off the lattice does not count), rows transposed into the store by its
 * catch-up k_vcol_build (index 19 vcol_rows_built)}; n <= 20. */
int mfgp_model_stats(const mfgp_model* m, int64_t* out, int n);
/* Tests only: the n = min(resident V rows, n_max) leading rows of V as doubles, v_out[i * M
 * + c] = V(i, c), and of the column store, vc_out[c * n + i] (either may be null);
 * *rows = n, *vc_rows = the store's valid rows (0: none). */
int mfgp_debug_read_v(mfgp_model* m, double* v_out, double* vc_out, int64_t n_max, int64_t* rows,
                      int64_t* vc_rows);
/* Tests only: the explicit inverse F = L^-1 that the lattice steps keep, its n = min(current
 * rows, n_max) leading rows and columns as doubles, f_out[i * n + j]; *rows = n (0: none). */
int mfgp_debug_read_f(mfgp_model* m, double* f_out, int64_t n_max, int64_t* rows);
/* Tests only: the memory the library holds in this process, out = {device buffers, their
 * bytes, pinned host buffers, their bytes}; the buffers of the view pool and of views not
 * yet released count. */
int mfgp_debug_live(int64_t out[4]);
/* Copy the lower Cholesky factor L [N,N] (row-major, zeros above the diagonal). */
int mfgp_get_factor(mfgp_model* m, double* L_out);

/* Batched update + predict over `count` independent GPs (Monte-Carlo seeds):
 * for model i append k[i] rows (rows of X/y, concatenated in model order),
 * refactor, and predict into mu + i*M_i, var + i*M_i (concatenated in model
 * order). One set of launches serves the whole batch. flags: MFGP_ASYNC. */
int mfgp_batch_append_predict(mfgp_model** models, int count, const double* X, const double* y,
                              const int64_t* k, double* mu, double* var, int flags);
/* A member with k[i] = 0 whose factor and resident posterior are current (it
 * was predicted before and nothing changed) is not recomputed: its outputs are its
 * resident posterior (the same bits as its last predict), copied by one launch for
 * all such members (device outputs; mfgp_model_stats counts them), and the step
 * runs over the others. */
/* mfgp_batch_append_predict plus fused reductions of each model's variance:
 * var_max[i] = np.amax of the posterior covariance (its largest diagonal entry,
 * simulator.py:672, 842, 1014) and var_argmax[i] = the first cell attaining it
 * (the argmax of compute_sample_points, sim:352). Either may be NULL; both are
 * device memory, written in stream order (no host round trip). */
int mfgp_batch_append_predict_ex(mfgp_model** models, int count, const double* X, const double* y,
                                 const int64_t* k, double* mu, double* var, double* var_max,
                                 int64_t* var_argmax, int flags);
/* The two halves of mfgp_batch_append_predict (append + refactor only; predict
 * from the current factors only). mfgp_batch_predict needs a current factor. */
int mfgp_batch_append_factor(mfgp_model** models, int count, const double* X, const double* y,
                             const int64_t* k, int flags);
int mfgp_batch_predict(mfgp_model** models, int count, double* mu, double* var, int flags);
/* compute_sample_points (simulator.py:326-374), the Choi planner's sample-set
 * selection, on the device: past the model's own rows (dropped at the end, with
 * what else the loop overwrote restored: the model is unchanged, no copy is made),
 * repeatedly append the grid cell of maximal posterior variance (first argmax)
 * with its posterior mean as the observation, until the maximal variance is
 * <= threshold or max_points points were chosen. points: [max_points, 2], host
 * or device; *count = points chosen. Each iteration is a 1-row bordered append
 * and a one-pass predict; the loop runs in chunks on the device (one host
 * synchronisation per 32 iterations). Needs the grid set and incremental
 * updates enabled. On any error (MFGP_ERR_NOT_PD from a step of the loop included)
 * the model is as before the call, and points / count are unspecified. */
int mfgp_sample_points(mfgp_model* model, double threshold, int64_t max_points, double* points, int64_t* count);
/* mfgp_sample_points for `count` models stepped together (the Choi planner of many
 * Monte-Carlo seeds, sim:326-374 once per seed): per iteration one decision launch
 * for all models and one batched 1-row append + predict (the lattice step where
 * the batch takes it); each model stops at its own thresholds[b] (host or device)
 * or after max_points points, and is unchanged (each appends past its own rows,
 * which are dropped and its state restored at the end). points:
 * [count][max_points][2], host or device; counts[b] = points chosen for model b.
 * The models share one context and dtype and need their grids set. On any error
 * (one model's step not positive definite included) every model is as before the
 * call, and points / counts are unspecified. */
int mfgp_batch_sample_points(mfgp_model** models, int count, const double* thresholds, int64_t max_points,
                             double* points, int64_t* counts);
/* The greedy integrated-variance planner: up to n_points grid cells chosen one after
 * another, each the allowed cell c that maximises the A-optimal score of
 * mfgp_var_reduction under one weight vector,
 *   sum_i w[i] cov_t(i, c)^2 / (cov_t(c, c) + noise_H + jitter),
 * where cov_t is the posterior covariance given the model's rows and the t cells
 * chosen before (each taken as a hifi row with the posterior mean at the cell as its
 * pseudo-observation). A pick changes the covariance by a rank-one term, so the scores
 * follow from one product of the covariance with a grid vector per pick (two streamed
 * passes over the resident V, mfgp_cov_apply's kernels) instead of mfgp_var_reduction's
 * GEMM: that GEMM runs once per call, and again after every `refresh` picks when
 * refresh > 0 (the numerators recomputed from scratch on the current rows: for long
 * runs, and the cross-check of the recurrence; 0 = never). w: [>= M] weights, ldw >= M,
 * host or device memory, NULL = ones. cand: a host array of the nc allowed cells in
 * [0, M), NULL = all cells (then nc must equal M); no other cell is ever chosen; among
 * equal scores the first position in the list wins, and a NaN score never does. The run
 * stops after n_points picks or before the first pick whose score is < min_gain. Outputs
 * (host memory): cells [n_points] the grid indices, points [n_points][2] their
 * coordinates, gains [n_points] each pick's score at the time it was chosen, *count the
 * number of picks. The loop runs on the model itself, past its own rows, in chunks of up
 * to 32 iterations behind a device gate with one status read per chunk, as
 * mfgp_sample_points; each append is the general batch step of one model (the lattice
 * step where its gates take it, else the fused V stream). The call settles the model as
 * mfgp_cov_block does (MFGP_ERR_NOT_PD, MFGP_ERR_NO_V as there) and validates everything
 * before anything is enqueued: a model without a grid, an MFGP_F32 model, ldw < M, a cell
 * outside [0, M), a non-finite weight in a host w, n_points < 0, refresh < 0, a null
 * output and a context with incremental updates disabled return MFGP_ERR_ARG, launch
 * nothing and leave the model as it was. n_points == 0 or nc == 0: MFGP_OK, *count = 0.
 * Afterwards -- and after any error, MFGP_ERR_NOT_PD from a step of the loop included --
 * the model is as the settling left it: its rows, its predict's bits and its path
 * counters (the loop's steps are counted in mfgp_ctx_planner_stats), and its next step
 * gives the bits of a model that never ran the planner. Two calls return the same cells
 * and the same gains bit for bit. */
int mfgp_plan_ivr(mfgp_model* m, const double* w, int64_t ldw, const int64_t* cand, int64_t nc,
                  int64_t n_points, double min_gain, int refresh,
                  int64_t* cells, double* points, double* gains, int64_t* count);
/* mfgp_plan_ivr for `count` models stepped together (a rank's Monte-Carlo seeds), with
 * per-group quotas on the picks ("one cell per agent"). Member b gets exactly the run
 * mfgp_plan_ivr describes, under its own weight row, candidate list, gate and stopping
 * point; per iteration there is one pick launch, one batched 1-row append + predict (as
 * mfgp_batch_sample_points) and one launch of each covariance-product kernel for the
 * whole batch. A member that stopped leaves the batch step at the next chunk boundary
 * (32 iterations; a refresh ends a chunk). The members are MFGP_F64 models of one context
 * with their grids set, none twice; their cell counts M_b and row counts may differ, and a
 * member without rows gives the prior's scores.
 *   w      [count][ldw] weights, row b for member b, ldw >= the largest M_b; host or device
 *          memory; NULL = ones.
 *   cand, cand_off   host: the members' candidate lists one after another, member b's at
 *          cand[cand_off[b] .. cand_off[b + 1]); cand_off has count + 1 entries, starts at 0
 *          and does not decrease. cand NULL = all cells of every member (cand_off is not
 *          read; member b's list is 0 .. M_b - 1 and the lists' offsets are the sums of M_b).
 *   group, quota, ngroups   host: group is parallel to the candidate lists: position j of
 *          member b belongs to group[offset_b + j] in [0, ngroups), ngroups in
 *          [1, MFGP_PLAN_MAXGROUPS]. A position is allowed at a pick iff its member has made
 *          fewer than quota[g] picks in its group so far; quota NULL = 1 each, quota[g] = 0
 *          bars a group. A cell may stand at several positions under different groups.
 *          group NULL = no constraint (quota must be NULL too).
 * Among equal scores the first allowed position wins, and a NaN score never does. A
 * member's run ends after n_points picks, before the first pick whose score is < min_gain,
 * or when no allowed position is left. Outputs (host memory), member b's at [b][..]:
 * cells [count][n_points], pos [count][n_points] (the chosen positions in the member's
 * list; NULL = not wanted), points [count][n_points][2], gains [count][n_points],
 * counts [count] the picks made. refresh as in mfgp_plan_ivr.
 * The call settles every member as mfgp_plan_ivr does (MFGP_ERR_NOT_PD, MFGP_ERR_NO_V) and
 * validates everything before anything is enqueued: count <= 0, a null output,
 * n_points < 0, refresh < 0, ldw less than the largest M_b, a cell outside its member's
 * grid, a group outside [0, ngroups), ngroups outside [1, MFGP_PLAN_MAXGROUPS] with group
 * set, a negative quota, cand_off not monotone from 0, a non-finite weight in a host w, an
 * MFGP_F32 member, a member without a grid, two contexts, a model twice and incremental
 * updates disabled return MFGP_ERR_ARG, launch nothing and leave all models as they were.
 * n_points == 0: MFGP_OK and zero counts. Afterwards, and after any error (one member's
 * step not positive definite included), every member is as the settling left it, with
 * mfgp_plan_ivr's guarantees: rows, predict bits and path counters as before, the loop's
 * steps counted in mfgp_ctx_planner_stats, the next step the bits of a twin that never ran
 * the planner. Two calls agree bit for bit. A member's sums are ordered by its own M alone,
 * so its covariance products do not depend on the batch; its appended rows are the batch
 * step's. */
#define MFGP_PLAN_MAXGROUPS 64
int mfgp_batch_plan_ivr(mfgp_model** models, int count, const double* w, int64_t ldw,
                        const int64_t* cand, const int64_t* cand_off,
                        const int32_t* group, const int64_t* quota, int ngroups,
                        int64_t n_points, double min_gain, int refresh,
                        int64_t* cells, int64_t* pos, double* points, double* gains, int64_t* counts);
/* Keep only the first n_keep_hifi hifi rows (no refactor; benchmark reset). */
int mfgp_truncate(mfgp_model* m, int64_t n_keep_hifi);
/* mfgp_truncate of count models with one call (the benchmark's per-step reset). */
int mfgp_batch_truncate(mfgp_model** models, int count, int64_t n_keep_hifi);

/* likelihood (gp:81-106 SF / gp:344-385 MF): the negative log-marginal
 * likelihood of the model's training data under the log-scaled hyperparameters
 * `hyp` (nhyp = 4 or 9; the model's own .hyp and factor are unchanged), and,
 * if grad != NULL, its gradient with respect to hyp ([nhyp]; the reference uses
 * autograd for it in train, gp:108-119 / 388-399). Unlike the data pointers of
 * the other entry points, `hyp`, `nlml` and `grad` are HOST memory: hyp is read
 * and *nlml / grad[] are written by the host. An empty model (N = 0) gives 0 and
 * a zero gradient. The factor is of a scratch model with the model's jitter as it
 * is set now (mfgp_model_set_hyp), on the model's context: a running launch of
 * that context is waited for, a staged (deferred) append stays staged and its rows
 * count. MFGP_ERR_NOT_PD as the reference's cholesky raising LinAlgError, and
 * MFGP_ERR_ARG for nhyp other than the model's. */
int mfgp_nlml(mfgp_model* m, const double* hyp, int nhyp, double* nlml, double* grad);

/* likelihood / its gradient (mfgp_nlml) for S hyperparameter vectors over the model's
 * data, in one set of launches per chunk of members (multi-start training, likelihood
 * surfaces). hyps [S][nhyp], nlml [S], grad [S][nhyp] or NULL, status [S] or NULL:
 * all HOST memory, as for mfgp_nlml, and the same preconditions: a running launch of
 * the context is waited for, the model's jitter as it is set now, a staged (deferred)
 * append stays staged and its rows count, an MFGP_F32 model is served in fp64, and
 * the model keeps its rows, serial, factor, resident V / posterior, kept predict
 * results and path counters.
 * Bit equality: member s's value and gradient are, bit for bit, what
 * mfgp_nlml(m, hyps + s * nhyp, nhyp, ..) returns. A member's bits therefore depend
 * on its own vector only: not on S, on its position, on the other members, on the
 * chunking (mfgp_ctx_set_nlml_chunk) or on whether grad was asked for.
 * status[s] = 0: success; > 0: the order of the leading minor of K(hyps[s]) that is
 * not positive definite (the number in mfgp_nlml's message); that member's nlml[s]
 * and gradient are NaN and the other members are served as usual. With status ==
 * NULL any such member makes the call return MFGP_ERR_NOT_PD, the outputs then
 * unspecified. A device error fails the whole call. S == 0: MFGP_OK, nothing
 * written. N = 0: value 0, a zero gradient and status 0 for every member.
 * MFGP_ERR_ARG for nhyp other than the model's (mfgp_nlml's message), S < 0, or NULL
 * hyps / nlml with S > 0. The members' scratch (factor storage, and L^-1 and K^-1 with
 * the gradient) lives with the context: grown on demand, reused by the next call,
 * given back by mfgp_ctx_trim / mfgp_ctx_destroy. */
int mfgp_nlml_batch(mfgp_model* m, const double* hyps, int S, int nhyp,
                    double* nlml, double* grad, int* status);

/* Voronoi-cell reductions over the grid (simulator.py:194-323). Cell i is the
 * closed polygon verts[vstart[i] .. vstart[i+1]) ([.,2], vertices of the
 * caller's bounded Voronoi region, sim:154-191; at most 256 per cell) with seed
 * seeds[i]. A grid point belongs to every cell whose polygon contains it by the
 * reference's in_polygon test (sim:105-124: matplotlib's crossing rule,
 * reproduced exactly). Per cell, out[6i .. 6i+6) = {points, sum w, sum w*x,
 * sum w*y, sum |x - seed|^2 * f, max var} and argmax[i] = first grid index of
 * the max var (-1 if the cell is empty). w (compute_centroids' mu, sim:231-283),
 * f (compute_loss' truth, sim:194-228) and var (compute_max_var, sim:286-323)
 * may each be NULL. Arrays may be host or device memory except vstart (host).
 * Synchronous. */
int mfgp_cell_reduce(mfgp_ctx* ctx, const double* grid, int64_t M, int ncells, const int* vstart,
                     const double* verts, const double* seeds, const double* w, const double* f,
                     const double* var, double* out, int64_t* argmax);

/* mfgp_cell_reduce over the partitions of several seeds in one launch (the
 * lockstep simulations of a seed batch, mfgp_coverage_amd/coverage.py: every
 * seed's loss partition of its agents and Lloyd partition of its centroids,
 * simulator.py:895-904). Cell i reads the fields of seed field[i]: w + field[i]*M
 * and var + field[i]*M (w and var are [nfield][M], e.g. the batch's posterior
 * means / variances as mfgp_batch_append_predict wrote them); f [M] is shared.
 * field and vstart are host memory. Same per-cell outputs as mfgp_cell_reduce
 * (bit for bit: a cell's reduction does not depend on the other cells).
 * Synchronous. */
int mfgp_batch_cell_reduce(mfgp_ctx* ctx, const double* grid, int64_t M, int ncells, const int* vstart,
                           const double* verts, const double* seeds, const int* field, int nfield,
                           const double* w, const double* f, const double* var, double* out, int64_t* argmax);

const char* mfgp_last_error(void);
const char* mfgp_version(void);

#ifdef __cplusplus
}
#endif

#endif /* MFGP_HIP_H */
