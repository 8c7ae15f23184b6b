// What the host translation units of libmfgp_hip.so share (host only; no kernel file
// includes it): error reporting, the device guard, the constants, the context and
// model state behind the C ABI's opaque handles, and the helpers that cross files.
//
//   mfgp_capi.hip      contexts, models, their state helpers, set / append / predict, stats
//   mfgp_step.hip      the step engine: enqueue_*, batch_run, the batch entry points
//   mfgp_planners.hip  the planner loops (sample points, batched, integrated variance) on
//                      one scaffold (PlanRun), and the cell reductions
//   mfgp_resident.hip  consumers of the resident V and factor: covariance blocks,
//                      variance reduction, look-ahead queries, pathwise samples; their
//                      shared argument checks (need_f64_grid, check_cells, finite_rows)
//   mfgp_train.hip     NLML and its gradient, single and batched
//
// The shared helpers live in mfgp_host, a namespace of hidden visibility: they link
// across the library's objects and add nothing to its dynamic symbol table. Matrices the
// caller may hold in host memory pass through StagedIn (inputs) and StagedOut (outputs).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstdint>
#include <memory>
#include <string>
#include <vector>

#include "../../include/mfgp_hip.h"
#include "mfgp_internal.h"
#include "mfgp_own.h"
#include "mfgp_state.h"

namespace mfgp_host __attribute__((visibility("hidden"))) {

// the thread's error string (mfgp_last_error); returns code
int set_err(int code, const char* fmt, ...);

#define HIP_TRY(expr)                                                                      \
  do {                                                                                     \
    hipError_t e_ = (expr);                                                                \
    if (e_ != hipSuccess) return mfgp_host::set_err(MFGP_ERR_DEVICE, "%s: %s (%s:%d)", #expr, \
                                                    hipGetErrorString(e_), __FILE__, __LINE__); \
  } while (0)

// The context's device for the duration of one entry point, the caller's restored on
// every return path (an entry point that set the device and left it
// changed torch.cuda.current_device() in a multi-GPU process). dev < 0: no change.
struct DeviceGuard {
  int prev = -1;
  explicit DeviceGuard(int dev) {
    if (dev < 0 || hipGetDevice(&prev) != hipSuccess) {
      prev = -1;
      return;
    }
    if (prev == dev || hipSetDevice(dev) != hipSuccess) prev = -1;
  }
  ~DeviceGuard() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
  DeviceGuard(const DeviceGuard&) = delete;
  DeviceGuard& operator=(const DeviceGuard&) = delete;
};

// ---- the device and pinned memory the library holds ----
// Every buffer of a context, a model or a record is a Dev<T> (hipFree) or a Pin<T>
// (hipHostFree); dev_alloc / pin_alloc are the only places that allocate, and the only
// ones that report a refused allocation. live_dev / live_pin count what is held
// (mfgp_debug_live), the view pool's buffers and handed-out views included.
extern mfgp_own::Live live_dev, live_pin;   // (mfgp_capi.hip)
inline void dev_free(void* p, size_t bytes) {
  (void)hipFree(p);
  live_dev.sub(bytes);
}
inline void pin_free(void* p, size_t bytes) {
  (void)hipHostFree(p);
  live_pin.sub(bytes);
}
template <class T>
using Dev = mfgp_own::Owner<T, dev_free>;
template <class T>
using Pin = mfgp_own::Owner<T, pin_free>;
// a refused allocation: HIP's last-error word cleared (the caller's next check of it, or
// PyTorch's, sees none), MFGP_ERR_DEVICE with the bytes asked for
inline int alloc_refused(const char* kind, size_t bytes) {
  (void)hipGetLastError();
  return set_err(MFGP_ERR_DEVICE, "out of %s memory: %zu bytes refused", kind, bytes);
}
enum : unsigned {
  A_ZERO = 1,      // zeroed on the stream
  A_2M = 2,        // whole 2 MiB units: small buffers that every GEMM workgroup of the lattice step
                   // reads (the axis tables, the member lists) sit in one large page
  A_NO_DRAIN = 4   // nothing enqueued reads o's old buffer (an empty or local owner)
};
// o's buffer replaced by a fresh one of `bytes` once the stream has drained (its launches
// may read the old one), the old one freed first. On failure o is empty: the caller resets
// the extent it keeps for o before the call, or commits it after.
template <class T>
int dev_alloc(Dev<T>& o, hipStream_t s, size_t bytes, unsigned flags = 0) {
  if (!(flags & A_NO_DRAIN)) HIP_TRY(hipStreamSynchronize(s));
  const size_t unit = size_t(2) << 20, want = (flags & A_2M) ? (bytes + unit - 1) / unit * unit : bytes;
  if (const int rc = mfgp_own::fill(
          o, want, live_dev, [](void** p, size_t b) { return (int)hipMalloc(p, b); },
          [](size_t b) { return alloc_refused("device", b); }))
    return rc;
  if ((flags & A_ZERO) && bytes > 0 && hipMemsetAsync(o.get(), 0, bytes, s) != hipSuccess) {
    o.reset();
    return set_err(MFGP_ERR_DEVICE, "zero fill of %zu bytes failed", bytes);
  }
  return MFGP_OK;
}
// the pinned twin (hip_flags: hipHostMallocDefault / Mapped / Portable); the caller drains
// the stream where launches may still write the old buffer
template <class T>
int pin_alloc(Pin<T>& o, size_t bytes, unsigned hip_flags) {
  return mfgp_own::fill(
      o, bytes, live_pin, [hip_flags](void** p, size_t b) { return (int)hipHostMalloc(p, b, hip_flags); },
      [](size_t b) { return alloc_refused("pinned host", b); });
}
// the device address of a mapped pinned buffer
template <class T>
int pin_device(const Pin<T>& o, T*& dev) {
  void* d = nullptr;
  HIP_TRY(hipHostGetDevicePointer(&d, o.get(), 0));
  dev = static_cast<T*>(d);
  return MFGP_OK;
}

constexpr int RING = 64;       // descriptor upload slots
constexpr int MAXB = 256;      // GPs per launch
constexpr int64_t MAX_FULL_CAP = 16319;   // largest training capacity the full predict serves (ld <= 16383)
constexpr size_t F32_SCRATCH = size_t(16) << 30;   // bytes of fp64 V scratch for MFGP_F32 full predicts
// bytes of scratch a chunk of mfgp_nlml_batch may hold (a member: its factor A, and Xi
// and Kv with the gradient, ld^2 doubles each): 40 members with the gradient at N = 2048
constexpr size_t NLML_BATCH_SCRATCH = size_t(4) << 30;
// lattice-separable step (k_inc_lat): taken when kss / (smallest noise + jitter)
// <= LAT_RMAX (its error grows with the conditioning of K),
// and for at most LAT_MAXD consecutive steps before var / mu are recomputed from V
constexpr double LAT_RMAX = 1e4;
constexpr int LAT_MAXD = 256;
// planner counters (mfgp_ctx_planner_stats): model runs, bordered appends, V-stream
// predicts, lattice steps (of them by value / with k_lat_gemm2), full factors, full
// predicts; then the batched planner's host time (us) before, in and after its loop
constexpr int PLAN_NSTATS = 11;

constexpr int STATUS_UNSET = INT_MIN + 1;   // status_host before the launch writes it

struct EvPair {
  hipEvent_t a, b;
  int kind;  // 0 predict, 1 factor
};

// The path counters of a model (mfgp_model::cnt). mfgp_model_stats reports them; a
// planner's loop saves and restores the whole array (PlanSave) and moves its steps to
// the context's planner counters by name, so a new counter is added here alone.
enum PathCounter {
  N_FULL_FACTOR,
  N_INC_FACTOR,
  N_FULL_PREDICT,
  N_VSTREAM,
  N_LATTICE,
  N_LATTICE_ARG,    // lattice steps launched with their descriptors by value (k_inc_lat_arg)
  N_LATTICE_G2,     // lattice steps whose GEMM and cells ran as a second launch (k_lat_gemm2)
  N_POST_COPY,      // batch predicts served from the resident posterior (k_post_copy: nothing appended)
  N_EARLY_PD,       // eager appends that returned at the launch's published L22 verdict
  N_LATTICE_VCOL,   // lattice steps whose w units read the store
  N_VCOL_ROWS,      // rows transposed into it by k_vcol_build (catch-up)
  N_LOOK_BORDER,    // k_look_border / k_look_query launches
  N_LOOK_QUERY,
  N_SAMPLE_SOLVE,   // k_sample_solve / k_sample_gemm launches
  N_SAMPLE_GEMM,
  N_COUNTERS
};

using mfgp_state::FactorLost;
using mfgp_state::Predict;

}  // namespace mfgp_host

struct mfgp_ctx {
  __attribute__((visibility("hidden"))) ~mfgp_ctx() = default;   // (not a symbol of the library)
  int device = 0;
  hipStream_t own = nullptr;
  hipStream_t stream = nullptr;
  // descriptor ring
  mfgp_host::Pin<mfgp::GPDesc> h_ring;  // pinned [RING][MAXB]
  mfgp_host::Dev<mfgp::GPDesc> d_ring;  // device [RING][MAXB]
  hipEvent_t ring_ev[mfgp_host::RING];
  bool ring_used[mfgp_host::RING];
  int ring_pos = 0;
  // workspace (V scratch + device outputs for host-pointer calls)
  mfgp_host::Dev<double> ws;   // (its extent: ws.bytes())
  // timing: 0 off, 1 predict + factor launches, 2 predict launches only
  int timing = 0;
  int64_t timing_stride = 1, timing_seq = 0;   // bracket every stride-th eligible launch
  std::vector<mfgp_host::EvPair> pending;
  std::vector<hipEvent_t> pool;
  double t_predict = 0.0, t_factor = 0.0;
  int64_t n_predict = 0, n_factor = 0;
  // deferred status words of ASYNC batches, with the model each belongs to (a
  // failed factor is dropped from its model at mfgp_ctx_synchronize)
  struct AsyncStatus {
    mfgp_model* m;
    int* dev;      // the model's status word (device; the model's, not owned here)
    int* host;     // its mapped host copy written by the launch (k_inc_stream1; the model's), or null: copy dev
  };
  std::vector<AsyncStatus> async_status;
  // fp64 scratch in which the full predicts of MFGP_F32 models compute V
  // (k_predict re-reads its own rows), then rounded into their fp32 V
  mfgp_host::Dev<double> vscr;   // (its extent: vscr.bytes())
  int f32_group = 1;          // full predicts per k_predict launch that share vscr
  // incremental append / predict (bordered Cholesky + resident V); off = always
  // refactor and recompute V from scratch, as the reference does
  bool incremental = true;
  bool fused = true;          // bordered append + one-pass predict in one launch (k_inc_stream)
  bool deferred = false;      // mfgp_append stages rows for a later (fused) bordered append
  bool lattice = true;        // lattice-separable appends (k_inc_lat) where they apply
  int lat_ksplit = 0;         // split-K of its GEMM tiles (0: chosen per launch; MFGP_LAT_KSPLIT, diagnostics)
  int lat_wu = 0;             // w units of a launch, all GPs (0: two per CU; MFGP_LAT_WU, diagnostics)
  int lat_selfg = -1;         // w units read L21 from V themselves (-1: for one GP; MFGP_LAT_SELFG, diagnostics)
  int lat_vcol = -1;          // the producers and the w units read L21 from the column store of V (Vc): -1 for a
                              // batch whose models all have one, 0 never (no store is allocated either), 1 the
                              // same as -1 (a model without a store cannot take it); MFGP_LAT_VCOL, tests, A/B runs
  int64_t vcol_budget = -1;   // bytes one model's store may take (-1: VCOL_MAX; 0: none; tests)
  int lat_gemm2 = -1;         // the step's GEMM and cells as a second launch (k_lat_gemm2): -1 where its
                              // tiles fill the chip once or twice, 1 always, 0 never (in-launch split-K
                              // tiles); MFGP_LAT_GEMM2, diagnostics and tests
  bool trinv_columns = false;  // F by the block-column k_trinv_f instead of recursive doubling (MFGP_TRINV_COLUMNS)
  int factor_depth = 4;        // 64-column steps per trailing-update pass of the factor (MFGP_FACTOR_DEPTH; 1: one-level)
  bool lat_force = false;     // take it for small batches too (mfgp_ctx_set_lattice(2): tests)
  // launches of this context may run concurrently with other contexts' (several
  // streams on one GPU, mfgp_ctx_set_concurrent): no launch may rely on all of its
  // workgroups being resident at once -- the lattice step's GEMM runs as the second
  // launch (k_lat_gemm2, no cross-workgroup waits) instead of in-launch split-K tiles
  bool concurrent = false;
  int rsplit_force = 0;       // one-pass predict row splits per cell group (0: the host's rule)
  int lat_zcsr = 1;           // the Z units read member lists built by one scan unit per part
                              // instead of bucketing every row themselves (MFGP_LAT_ZCSR=0: off)
  int plan_sep = 1;           // the covariance products take the separable K** x on lattice grids
                              // (MFGP_PLAN_SEP=0: always the general form; tests)
  int64_t spin_us = 2000;     // host polling of mapped status words before a synchronise (MFGP_SPIN_US; 0: off)
  // the eager append of one GP (spec_append_predict) returns at the step's L22
  // verdict, published by the launch as soon as it is known, instead of at the
  // launch's end: the caller's host work until its next call (the simulator's
  // grid check, the predict's argument handling) overlaps the posterior
  // (MFGP_EARLY_PD=0: wait for the launch's end)
  bool early_pd = true;
  bool early_running = false;  // such a launch may still run: the next entry point settles it first
  bool desc_arg = true;       // a batch step that is one k_inc_lat / k_inc_stream launch passes its
                              // descriptors by value
                              // (MFGP_DESC_ARG=0: upload them, diagnostics)
  // pinned host staging of the status words
  mfgp_host::Pin<int> h_status;   // (bytes() / sizeof(int) words)
  // mfgp_nlml_batch: members per set of launches (0: as many as NLML_BATCH_SCRATCH
  // holds) and its scratch (NlmlLayout), grown on demand, kept for the next call and
  // given back by mfgp_ctx_trim
  int nlml_chunk = 0;
  mfgp_host::Dev<double> nb_dev;    // (their extents: bytes())
  mfgp_host::Pin<double> nb_host;

  int ncu = 256;              // compute units (hipDeviceProp multiProcessorCount)
  // the path counters of the planners' loops (mfgp_sample_points,
  // mfgp_batch_sample_points), moved here from the models when each loop ends:
  // which step form the Choi iterations took (mfgp_ctx_planner_stats)
  int64_t plan_stats[mfgp_host::PLAN_NSTATS] = {0};
};

// The look-ahead record of a model (mfgp_query): the border of its last prospective
// set, keyed by the model's serial and the set's rows and fidelities.
struct mfgp_look_rec {
  __attribute__((visibility("hidden"))) ~mfgp_look_rec() = default;   // (not a symbol of the library)
  mfgp_host::Dev<double> W;      // [wld][64]: L^-1 K(X, X_P)
  int64_t wld = 0;
  mfgp_host::Dev<double> L22;    // [64][64] | L22inv [64][64] | ppts [64][2] (one allocation)
  mfgp_host::Dev<int> pfid;      // [64] fidelities, then the border's status word
  bool valid = false;        // the border below is stored for (serial, P, key)
  uint64_t serial = 0;
  int P = 0;
  std::vector<double> key;   // the P rows (x, y), then their fidelities
};

// The sample record of a model (mfgp_sample_posterior): the pivoted-Cholesky factors of
// the lattice axes' Gram matrices per field, keyed by the model's serial, and the
// lattice indices of its training rows.
struct mfgp_sample_rec {
  __attribute__((visibility("hidden"))) ~mfgp_sample_rec() = default;   // (not a symbol of the library)
  bool valid = false;        // the axis factors below belong to `serial`
  uint64_t serial = 0;
  int fields = 0, nx = 0, ny = 0;
  int rx[2] = {0, 0}, ry[2] = {0, 0};
  mfgp_host::Dev<double> fac;   // device: per field Ax [nx][rx] | AyT [ry][ny]
  size_t fac_n = 0;          // doubles allocated
  size_t off_ax[2] = {0, 0}, off_ay[2] = {0, 0};
  mfgp_host::Dev<int> lidx;     // device [lidx_cap]: px | (py << 16) per training row
  int64_t lidx_cap = 0;
  bool lidx_valid = false;   // lidx holds the N rows of `lidx_serial`
  uint64_t lidx_serial = 0;
  int64_t off_row = -1;      // the first training row that is no cell of the lattice, or -1
};

struct mfgp_model {
  // (not a symbol of the library) every buffer below frees itself; the two records are the model's
  __attribute__((visibility("hidden"))) ~mfgp_model() {
    delete look;
    delete samp;
  }
  mfgp_ctx* ctx = nullptr;
  // device gate of every step of this model (the planners' loops: 0 = skip); points into
  // the running planner's state, not owned
  int* gate_dev = nullptr;
  int kind = MFGP_SF;
  int dtype = MFGP_F64;     // precision of the resident V (MFGP_F32: fp32 storage and stream)
  int nhyp = 4;
  double hyp[9] = {0};
  double jitter = 1e-8;
  // training set (device)
  int64_t NL = 0, NH = 0, cap = 0;
  mfgp_host::Dev<double> X;  // [cap,2]
  mfgp_host::Dev<double> y;  // [cap]
  // factor (device)
  int64_t ld = 0;
  mfgp_host::Dev<double> A;     // [ld,ld]
  mfgp_host::Dev<double> Linv;  // [ld/NB][TILE]
  mfgp_host::Dev<double> zv;     // [cap] z = L^-1 (y - m)
  mfgp_host::Dev<double> iscr;   // incremental-append scratch (inc_scratch_doubles(cap))
  mfgp_host::Dev<int> status;
  mfgp_host::Pin<int> status_host;       // mapped pinned words the single-GP fused launch publishes into:
                                    // [0] its status (last act), [1] the L22 verdict (pd_host)
  int* status_host_dev = nullptr;   // its device address (an alias of status_host, not owned)
  // which rows of the derived buffers below are current (the factor, V, the compact rows,
  // F, the tables, the column store, the resident posterior): mfgp_state.h, the one place
  // that changes it
  mfgp_state::ModelState st;
  // grid (device)
  int64_t M = 0, Mcap = 0;
  mfgp_host::Dev<double> grid;
  mfgp::GridLattice lat{};        // lattice structure of the grid (nx == 0: none)
  std::vector<double> hax, hay;   // the lattice's axis values (host copy, for rows_on_cells)
  // resident V = L^-1 psi^T [vtiles][vld][PBM] (double, or float for MFGP_F32);
  // rows [0, st.v_n) valid for the current factor and grid
  mfgp_host::Dev<void> V;
  int64_t vld = 0, vtiles = 0;
  mfgp_host::Dev<double> tred;     // [vtiles][2] per-tile (max, argmax) of var, then the tiles' arrival counter
  int64_t tred_n = 0;         // doubles of tred
  mfgp_host::Dev<unsigned> sync;   // k_inc_stream hand-off words {arrivals, L21 ready, L22 ready} (zeroed)
  unsigned epoch = 0;         // last k_inc_stream epoch of this model
  // (the compact bordered rows in iscr, inc_l21c_offset: rows [st.l21c_n0, st.l21c_N)
  // bordered onto st.l21c_n0 factor rows)
  // speculative predict: an (eager) append that follows the pattern append ->
  // predict runs the bordered append and the one-pass predict as one launch and
  // keeps mu | var in `spec_out` (mapped pinned, [2][M]) for the predict that
  // follows; any change to the model drops them
  mfgp_host::Pin<double> spec_out;
  double* spec_out_dev = nullptr;   // its device address (an alias of spec_out, not owned)
  int64_t spec_cap = 0;
  bool spec_valid = false;
  // spec_out's trailer [2 cap] = (max var, its first argmax) holds the fused var
  // max / argmax of the launch that wrote spec_out (the eager append's): the
  // drop-in's np.amax / np.argmax of the covariance read it instead of rescanning
  bool spec_max = false;
  bool pred_since_append = false;   // a predict came after the last append
  // path counters (mfgp_model_stats), indexed by PathCounter
  int64_t cnt[mfgp_host::N_COUNTERS] = {0};
  mfgp_look_rec* look = nullptr;   // look-ahead record (allocated by the first mfgp_query, not cloned)
  mfgp_sample_rec* samp = nullptr;   // sample record (allocated by the first mfgp_sample_*, not cloned)
  mfgp_host::Dev<unsigned> csr;     // the scan units' member lists (csr_bytes; mfgp_internal.h)
  // posterior serial (mfgp_model_serial): a process-wide fresh value at every change
  // of the rows, hyperparameters, jitter or grid -- unlike (gen, N) it never repeats
  // (truncate + append of the same count), so a holder of an earlier predict's
  // result can tell whether the model still holds that posterior
  uint64_t serial = 0;
  // resident posterior: two buffers [mu | var] of M each, written by every predict
  // (incremental mode); buffer b holds the posterior of the st.res[b].n leading rows
  mfgp_host::Dev<double> res;
  int64_t res_M = 0;
  // lattice-separable step state (allocated on first use)
  mfgp_host::Dev<double> F;        // explicit L^-1 [F_ld][F_ld], rows st.F
  mfgp_host::Dev<float> Ff;        // MFGP_F32: F in fp32 (the rows the lattice steps stream and extend)
  int64_t F_ld = 0;
  mfgp_host::Dev<double> tab;      // separable tables [4][tab_ld][tabw], rows st.tab
  int64_t tab_ld = 0, tabw = 0;
  mfgp_host::Dev<double> wv;       // w [wv_ld][KINC]
  int64_t wv_ld = 0;
  mfgp_host::Dev<unsigned> wflag;  // [wv_ld / 64 + 2]
  mfgp_host::Dev<unsigned> wcnt;   // [wv_ld / 64 + 2]
  mfgp_host::Dev<double> wpart;    // [LAT_WU_MAX + wv_ld / 64 + 1][1024]
  mfgp_host::Dev<double> gpart;    // split-K partials
  size_t gpart_n = 0;
  mfgp_host::Dev<unsigned> gcnt;   // per GEMM tile
  int64_t gcnt_n = 0;
  mfgp_host::Dev<int> lidx;   // lattice indices per training row [tab_ld], rows st.tab (with the tables)
  mfgp_host::Dev<double> axt;      // axis tables [4][tabw + 1][tabw], current for generation st.axt_gen
  int64_t axt_w = 0;
  mfgp_host::Dev<double> zb;       // Z rows [P][zrows][tabw][zb_ka]
  int64_t zb_rows = 0, zb_w = 0;
  int zb_ka = 0;
  mfgp_host::Dev<unsigned> zflag;  // [zflag_n]
  int64_t zflag_n = 0;
  mfgp_host::Dev<unsigned> ldone;  // [4] lattice phase hand-offs (arrivals | flag, twice)
  mfgp_host::Dev<int> zvl;         // [2][zb_rows + 1]
  // the column store of V, Vc[cell][vc_ld] in V's element type: rows st.vc equal V's
  // (allocated with the lattice state where the budget allows: ensure_vcol)
  mfgp_host::Dev<void> Vc;
  int64_t vc_ld = 0, vc_M = 0;
  int64_t vc_deny_ld = -1, vc_deny_M = -1, vc_deny_budget = -2;   // the shape and budget last refused
};

namespace mfgp_host __attribute__((visibility("hidden"))) {

inline int64_t round_up(int64_t a, int64_t b) { return (a + b - 1) / b * b; }

// A model destroyed with the scope unless release()d: one under construction
// (mfgp_model_create, mfgp_clone), a scratch model (mfgp_nlml).
struct ModelDestroy {
  void operator()(mfgp_model* m) const { mfgp_model_destroy(m); }
};
using ModelGuard = std::unique_ptr<mfgp_model, ModelDestroy>;

// An eager append that returned at its L22 verdict (mfgp_ctx::early_pd) may still
// run: every entry point waits for it, and takes its status, before it reads or
// reuses anything the launch touches.
inline int settle(mfgp_ctx* c) { return (c && c->early_running) ? mfgp_ctx_synchronize(c) : MFGP_OK; }

int check_model(const mfgp_model* m);

// The opening of an entry point on one model: the context's device (restored when the
// entry point returns), then the running eager append settled, then the model checked;
// rc is the first failure of the two.
struct Entry {
  const DeviceGuard dg_;
  int rc;
  explicit Entry(const mfgp_model* m) : dg_(m ? m->ctx->device : -1), rc(settle(m ? m->ctx : nullptr)) {
    if (rc == MFGP_OK) rc = check_model(m);
  }
};

// Offsets of the pieces of a workspace, in the order they are taken, each rounded up
// to 256 bytes; `end` is the room they need.
struct WsLayout {
  size_t end = 0;
  static size_t up(size_t bytes) { return (bytes + 255) / 256 * 256; }
  size_t take(size_t bytes) {
    const size_t at = end;
    end += up(bytes);
    return at;
  }
};

// An output matrix of `cols` columns that the caller may hold in host memory: the
// kernels write `dev` with leading dimension `ld` -- the caller's buffer and ldo when
// it is device memory, else the packed image at `stage` (workspace), which copy_back
// enqueues into the caller's buffer. The caller synchronises.
struct StagedOut {
  double* dev;
  int64_t ld;
  double* user;   // the host buffer copy_back fills (null: nothing to copy)
  int64_t user_ld;
  StagedOut(double* out, int64_t ldo, bool host, void* stage, int64_t cols)
      : dev(host ? static_cast<double*>(stage) : out), ld(host ? cols : ldo), user(host ? out : nullptr), user_ld(ldo) {}
  hipError_t copy_back(int64_t cols, int64_t rows, hipStream_t s) const {
    if (!user) return hipSuccess;
    return hipMemcpy2DAsync(user, sizeof(double) * user_ld, dev, sizeof(double) * ld, sizeof(double) * cols, rows,
                            hipMemcpyDeviceToHost, s);
  }
};

// The input-side twin: a matrix [rows][cols] with leading dimension ldp that the kernels
// read at `dev` with leading dimension `ld` -- in place when it is device memory, else from
// the packed image at `stage` (workspace) that upload enqueues.
struct StagedIn {
  const double* dev;
  int64_t ld;
  const double* user;   // the host matrix upload copies (null: nothing to copy)
  int64_t user_ld, rows;
  StagedIn(const double* p, int64_t rows, int64_t cols, int64_t ldp, bool host, void* stage)
      : dev(host ? static_cast<const double*>(stage) : p), ld(host ? cols : ldp), user(host ? p : nullptr), user_ld(ldp),
        rows(rows) {}
  hipError_t upload(hipStream_t s) const {
    if (!user) return hipSuccess;
    return hipMemcpy2DAsync(const_cast<double*>(dev), sizeof(double) * ld, user, sizeof(double) * user_ld,
                            sizeof(double) * ld, rows, hipMemcpyHostToDevice, s);
  }
};

// table width of the lattice step: 64, 128, 192 or 256 where the step applies (lat_eligible:
// <= NT). At 192 zq rounds down to 2 and a Z unit's second thread group is a partial one
// (lat_zunit); every width, rectangles and a degenerate axis: tests/test_gpu_lattice_grids.py
inline int64_t lat_tabw(const mfgp_model* m) { return round_up(std::max<int64_t>(m->lat.nx, m->lat.ny), 64); }

// mfgp_capi.hip: state
void bump_serial(mfgp_model* m);
mfgp::Hyp derive_hyp(int kind, const double* hyp, double jitter);
int ensure_h_status(mfgp_ctx* c, size_t n);
int ensure_ws(mfgp_ctx* c, size_t bytes);
int ensure_cap(mfgp_model* m, int64_t need);
int ensure_v(mfgp_model* m);
void fill_desc(mfgp::GPDesc& d, mfgp_model* m);
double* res_mu(mfgp_model* m, int b);
double* res_var(mfgp_model* m, int b);
int res_find(const mfgp_model* m, int64_t n);
int set_res_out(mfgp_model* m, mfgp::GPDesc& d, int keep);
int ensure_lat(mfgp_model* m, int64_t tiles, int ksplit, int ka, int64_t nzu);
int ensure_vcol(mfgp_model* m);
int64_t vcol_rows(const mfgp_model* m);
int status_error(int st);
int read_status(mfgp_model* m);
int ensure_spec_out(mfgp_model* m);
bool factor_current(const mfgp_model* m);
bool can_inc_factor(const mfgp_model* m);
bool can_vstream(const mfgp_model* m);
bool is_device_ptr(const void* p);
int copy_rows(mfgp_model* m, int64_t at, const double* X, const double* y, int64_t k);

// mfgp_step.hip: descriptor slots, launches, the batch step
mfgp::GPDesc* acquire_slot(mfgp_ctx* c, int& slot, int& rc);
int upload_slot(mfgp_ctx* c, int slot, int count, const mfgp::GPDesc** dptr);
int release_slot(mfgp_ctx* c, int slot);
int enqueue_factor(mfgp_ctx* c, const mfgp::GPDesc* dd, const mfgp::GPDesc* hd, int count);
int enqueue_vstream(mfgp_ctx* c, const mfgp::GPDesc* dd, const mfgp::GPDesc* hd, int count);
int enqueue_predict(mfgp_ctx* c, const mfgp::GPDesc* dd, const mfgp::GPDesc* hd, int count);
int assign_predict_scratch(mfgp_ctx* c, mfgp::GPDesc* hd, int count);
void set_rsplit(const mfgp_ctx* c, mfgp::GPDesc* hd, int count);
void mark_inc_factor(mfgp_model* m);
int fill_inc_desc(mfgp::GPDesc& d, mfgp_model* m);
void set_vstream_rows(mfgp::GPDesc& d, const mfgp_model* m);
int factor_one(mfgp_model* m);
int update_factor(mfgp_model* m);
int batch_run(mfgp_model** models, int count, const double* X, const double* y, const int64_t* k, double* mu,
              double* var, double* vmax, int64_t* vargmax, int flags, bool do_factor, bool do_predict,
              const int64_t* out_offs = nullptr, const int* vidx = nullptr);

// mfgp_resident.hip
bool all_finite(const double* p, int64_t n);
int ensure_resident_v(mfgp_model* m, const char* who);
// The argument checks the consumers of the resident V share (`who`: the entry point, for
// the message). need_f64_grid: an fp64 model with a grid. check_cells: a NULL list stands
// for all M cells and n must say so; the entries of any other lie in [0, M).
// finite_rows: the first of p's rows ([rows][cols], leading dimension ld) with a
// non-finite entry, or -1.
int need_f64_grid(const mfgp_model* m, const char* who);
int check_cells(const char* who, const char* name, const int64_t* list, int64_t n, int64_t M);
int64_t finite_rows(const double* p, int64_t rows, int64_t ld, int64_t cols);
// The scratch and the fixed arguments of covariance products u = K** x - V^T (V x) on
// m's grid (mfgp_plan_ivr.hip): laid out at `base` (cov_work_bytes(m, rows) bytes, 256-byte
// aligned, for a V of at most `rows` rows). cov_work_init enqueues the axis Gram matrices
// of the separable K** x where the grid is a lattice it serves; cov_work_run enqueues one
// product from the model's current V (a.x, a.u or a.S / a.g / a.tau_part / a.ntau and
// a.gate set by the caller; n_rows: the rows of V that enter).
struct CovWork {
  mfgp::CovApply a;
  mfgp::KssArgs k;
  bool sep = false;
  double* T = nullptr;
  double* kx = nullptr;
};
size_t cov_work_bytes(const mfgp_model* m, int64_t rows);
int cov_work_init(mfgp_model* m, char* base, int64_t rows, CovWork& w);
int cov_work_run(mfgp_model* m, CovWork& w, int64_t n_rows);

}  // namespace mfgp_host

// (an exported symbol of the library since the eager append: kept)
extern "C" int spec_append_predict(mfgp_model* m, const double* X, const double* y, int64_t k);
