// Consumers of the resident V and factor: posterior covariance blocks (mfgp_cov.hip),
// integrated variance reduction (mfgp_ivr.hip), look-ahead and off-grid queries
// (mfgp_look.hip) and pathwise samples (mfgp_sample.hip). Each brings V over all N
// rows first (ensure_resident_v), lays its scratch out in the context's workspace
// (WsLayout) and stages matrices the caller holds in host memory there (StagedIn,
// StagedOut). The argument checks they share are need_f64_grid, check_cells, finite_rows.
#include <cmath>
#include <cstring>

#include "mfgp_host.h"

using namespace mfgp;
using namespace mfgp_host;

namespace mfgp_host __attribute__((visibility("hidden"))) {   // (as in mfgp_host.h: the definitions too)

// V holds all N rows of the current factor, hyperparameters and grid: the state
// every predict path leaves (mfgp_cov_block reads rows [0, N) of it).
static bool v_covers(const mfgp_model* m) {
  return m->st.v_covers(m->NL + m->NH, m->hyp, m->jitter) && m->V && m->vtiles >= ntiles_grid(m->M);
}

// Bring V over all N rows, as mfgp_predict would (a pending or deferred append, new
// hyperparameters, a new grid): into the model's result buffer, kept for the next
// predict. `who`: the entry point, for the error message.
int ensure_resident_v(mfgp_model* m, const char* who) {
  int rc;
  if (m->NL + m->NH == 0 || v_covers(m)) return MFGP_OK;
  if ((rc = ensure_spec_out(m))) return rc;
  m->spec_valid = false;   // (a kept result without its V is of no use here: recompute)
  if ((rc = mfgp_predict(m, m->spec_out, m->spec_out + m->spec_cap))) return rc;
  if (!v_covers(m))
    return set_err(MFGP_ERR_NO_V, "%s: the resident V holds %lld of the model's %lld rows after a predict", who,
                   (long long)m->st.v_n, (long long)(m->NL + m->NH));
  return MFGP_OK;
}

bool all_finite(const double* p, int64_t n) {
  for (int64_t i = 0; i < n; ++i)
    if (!std::isfinite(p[i])) return false;
  return true;
}

int need_f64_grid(const mfgp_model* m, const char* who) {
  if (m->dtype != MFGP_F64)
    return set_err(MFGP_ERR_ARG, "%s: MFGP_F32 models (fp32 V) are not supported; use an MFGP_F64 model", who);
  if (m->M <= 0 || !m->grid) return set_err(MFGP_ERR_ARG, "%s: the model has no grid (mfgp_set_grid)", who);
  return MFGP_OK;
}

int check_cells(const char* who, const char* name, const int64_t* list, int64_t n, int64_t M) {
  if (!list && n != M)
    return set_err(MFGP_ERR_ARG, "%s: a NULL candidate list means all %lld cells (got nc = %lld)", who, (long long)M,
                   (long long)n);
  for (int64_t i = 0; list && i < n; ++i)
    if (list[i] < 0 || list[i] >= M)
      return set_err(MFGP_ERR_ARG, "%s: %s[%lld] = %lld is outside the grid's cells [0, %lld)", who, name, (long long)i,
                     (long long)list[i], (long long)M);
  return MFGP_OK;
}

int64_t finite_rows(const double* p, int64_t rows, int64_t ld, int64_t cols) {
  for (int64_t r = 0; r < rows; ++r)
    if (!all_finite(p + r * ld, cols)) return r;
  return -1;
}

// K** x by the axis products: a lattice grid with both axes within KSS_AXIS_MAX
static bool kss_separable(const mfgp_model* m) {
  const GridLattice& L = m->lat;
  return m->ctx->plan_sep && L.nx > 0 && L.ny > 0 && L.nx <= KSS_AXIS_MAX && L.ny <= KSS_AXIS_MAX &&
         (int64_t)L.nx * L.ny == m->M;
}

// [part [segments][rows] | p [rows] | ax, ay | T [parts][M] | kx [M]]
size_t cov_work_bytes(const mfgp_model* m, int64_t rows) {
  WsLayout lay;
  const int64_t r = std::max<int64_t>(rows, 1);
  lay.take(sizeof(double) * (size_t)cov_segments(m->M) * r);
  lay.take(sizeof(double) * (size_t)r);
  if (kss_separable(m)) {
    const size_t parts = m->kind == MFGP_SF ? 1 : 2;
    lay.take(sizeof(double) * parts * ((size_t)m->lat.nx * m->lat.nx + (size_t)m->lat.ny * m->lat.ny));
    lay.take(sizeof(double) * parts * (size_t)m->M);
    lay.take(sizeof(double) * (size_t)m->M);
  }
  return lay.end;
}

int cov_work_init(mfgp_model* m, char* base, int64_t rows, CovWork& w) {
  WsLayout lay;
  const int64_t r = std::max<int64_t>(rows, 1);
  w = CovWork{};
  w.a.part = reinterpret_cast<double*>(base + lay.take(sizeof(double) * (size_t)cov_segments(m->M) * r));
  w.a.pld = r;
  w.a.p = reinterpret_cast<double*>(base + lay.take(sizeof(double) * (size_t)r));
  w.a.M = m->M;
  w.a.grid = m->grid;
  w.a.h = derive_hyp(m->kind, m->hyp, m->jitter);
  w.sep = kss_separable(m);
  if (!w.sep) return MFGP_OK;
  const GridLattice& L = m->lat;
  KssArgs& k = w.k;
  k.grid = m->grid;
  k.nx = L.nx;
  k.ny = L.ny;
  k.sx = L.sx;
  k.sy = L.sy;
  k.parts = m->kind == MFGP_SF ? 1 : 2;
  k.h = w.a.h;
  const size_t nx2 = (size_t)L.nx * L.nx, ny2 = (size_t)L.ny * L.ny;
  k.ax = reinterpret_cast<double*>(base + lay.take(sizeof(double) * k.parts * (nx2 + ny2)));
  k.ay = k.ax + k.parts * nx2;
  w.T = reinterpret_cast<double*>(base + lay.take(sizeof(double) * k.parts * (size_t)m->M));
  w.kx = reinterpret_cast<double*>(base + lay.take(sizeof(double) * (size_t)m->M));
  HIP_TRY(launch_kss_axes(k, m->ctx->stream));
  return MFGP_OK;
}

int cov_work_run(mfgp_model* m, CovWork& w, int64_t n_rows) {
  if (n_rows > w.a.pld) return set_err(MFGP_ERR_DEVICE, "covariance product: %lld rows exceed the scratch's %lld",
                                       (long long)n_rows, (long long)w.a.pld);
  w.a.V = static_cast<const double*>(m->V.get());
  w.a.vld = m->vld;
  w.a.N = n_rows;
  w.a.kx = nullptr;
  if (w.sep) {
    HIP_TRY(launch_kss(w.k, w.a.x, w.T, w.kx, w.a.gate, m->ctx->stream));
    w.a.kx = w.kx;
  }
  HIP_TRY(launch_cov_apply(w.a, m->ctx->stream));
  return MFGP_OK;
}

}  // namespace mfgp_host

extern "C" {

int mfgp_cov_block(mfgp_model* m, const int64_t* rows, int64_t na, const int64_t* cols, int64_t nb, double* out,
                   int64_t ldo, int flags) {
  const Entry entry(m);
  int rc = entry.rc;
  if (rc) return rc;
  mfgp_ctx* c = m->ctx;
  if ((rc = need_f64_grid(m, "mfgp_cov_block"))) return rc;
  if (na < 0 || nb < 0) return set_err(MFGP_ERR_ARG, "mfgp_cov_block: negative block size");
  if ((!rows && na != m->M) || (!cols && nb != m->M))
    return set_err(MFGP_ERR_ARG, "mfgp_cov_block: a NULL index list means all %lld cells (got na = %lld, nb = %lld)",
                   (long long)m->M, (long long)na, (long long)nb);
  if (na == 0 || nb == 0) return MFGP_OK;
  if (!out) return set_err(MFGP_ERR_ARG, "mfgp_cov_block: null output");
  if (ldo < nb)
    return set_err(MFGP_ERR_ARG, "mfgp_cov_block: ldo = %lld is less than nb = %lld", (long long)ldo, (long long)nb);
  if ((na + 63) / 64 > 65535) return set_err(MFGP_ERR_ARG, "mfgp_cov_block: at most %d rows per call", 65535 * 64);
  if ((rc = check_cells("mfgp_cov_block", "rows", rows, na, m->M)) ||
      (rc = check_cells("mfgp_cov_block", "cols", cols, nb, m->M)))
    return rc;
  const bool prior = (flags & MFGP_COV_PRIOR) != 0;
  if (!prior && (rc = ensure_resident_v(m, "mfgp_cov_block"))) return rc;
  // workspace: [rows | cols | the block, when out is host memory]
  const bool host = !is_device_ptr(out);
  WsLayout lay;
  const size_t o_idx = lay.take(sizeof(int64_t) * (size_t)((rows ? na : 0) + (cols ? nb : 0)));
  const size_t o_out = lay.take(host ? sizeof(double) * (size_t)na * nb : 0);
  if ((rc = ensure_ws(c, lay.end))) return rc;
  char* ws = reinterpret_cast<char*>(c->ws.get());
  int64_t* drows = rows ? reinterpret_cast<int64_t*>(ws + o_idx) : nullptr;
  int64_t* dcols = cols ? reinterpret_cast<int64_t*>(ws + o_idx) + (rows ? na : 0) : nullptr;
  if (rows) HIP_TRY(hipMemcpyAsync(drows, rows, sizeof(int64_t) * na, hipMemcpyHostToDevice, c->stream));
  if (cols) HIP_TRY(hipMemcpyAsync(dcols, cols, sizeof(int64_t) * nb, hipMemcpyHostToDevice, c->stream));
  const StagedOut so(out, ldo, host, ws + o_out, nb);
  GPDesc d;
  fill_desc(d, m);
  HIP_TRY(launch_cov_block(d, drows, na, dcols, nb, so.dev, so.ld, (prior || d.N == 0) ? 1 : 0, c->stream));
  HIP_TRY(so.copy_back(nb, na, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return MFGP_OK;
}

// Look-ahead variance and off-grid queries (mfgp_look.hip). Queries run in chunks of
// LOOK_CHUNK points (one k_look_query launch each) unless the covariance is wanted,
// whose GEMM reads every tile of one scratch.
constexpr int64_t LOOK_CHUNK = 16384;

// Integrated variance reduction per candidate cell (mfgp_ivr.hip): k_cov_block's GEMM
// over the resident V with the column sums of w o cov^2 kept in registers.
int mfgp_var_reduction(mfgp_model* m, const int64_t* cand, int64_t nc, const double* w, int nw, int64_t ldw,
                       double* out, int64_t ldo, double* best, int64_t* best_pos) {
  const Entry entry(m);
  int rc = entry.rc;
  if (rc) return rc;
  mfgp_ctx* c = m->ctx;
  const int64_t M = m->M;
  if ((rc = need_f64_grid(m, "mfgp_var_reduction"))) return rc;
  if (nc < 0) return set_err(MFGP_ERR_ARG, "mfgp_var_reduction: negative candidate count");
  if (!cand && (rc = check_cells("mfgp_var_reduction", "cand", nullptr, nc, M))) return rc;   // (the entries: below)
  if (nw < 1 || nw > MFGP_IVR_MAXW)
    return set_err(MFGP_ERR_ARG, "mfgp_var_reduction: nw = %d is outside [1, %d]", nw, MFGP_IVR_MAXW);
  if (!w && nw != 1)
    return set_err(MFGP_ERR_ARG, "mfgp_var_reduction: NULL weights mean one vector of ones (got nw = %d)", nw);
  if (w && ldw < M)
    return set_err(MFGP_ERR_ARG, "mfgp_var_reduction: ldw = %lld is less than M = %lld", (long long)ldw, (long long)M);
  if (ldo < nc)
    return set_err(MFGP_ERR_ARG, "mfgp_var_reduction: ldo = %lld is less than nc = %lld", (long long)ldo, (long long)nc);
  if (ivr_segments(M) > 65535)
    return set_err(MFGP_ERR_ARG, "mfgp_var_reduction: grids of at most %lld cells are supported",
                   (long long)65535 * IVR_SEG * PBM);
  if ((rc = check_cells("mfgp_var_reduction", "cand", cand, nc, M))) return rc;
  const bool w_host = w && !is_device_ptr(w);
  if (const int64_t k = w_host ? finite_rows(w, nw, ldw, M) : -1; k >= 0)
    return set_err(MFGP_ERR_ARG, "mfgp_var_reduction: the weights must be finite (vector %d)", (int)k);
  if (nc == 0) return MFGP_OK;
  if (!out) return set_err(MFGP_ERR_ARG, "mfgp_var_reduction: null output");
  if ((rc = ensure_resident_v(m, "mfgp_var_reduction"))) return rc;
  // workspace: [cand | host weights [nw][M] | partial | out, when it is host memory | the
  // workgroups' maxima and positions | best | best_pos], each 256-byte aligned
  const bool o_host = !is_device_ptr(out);
  const bool want_best = best || best_pos;
  const int64_t nseg = ivr_segments(M), nblk = ivr_finish_blocks(nc);
  WsLayout lay;
  const size_t o_cand = lay.take(cand ? sizeof(int64_t) * (size_t)nc : 0);
  const size_t o_w = lay.take(w_host ? sizeof(double) * (size_t)nw * M : 0);
  const size_t o_part = lay.take(sizeof(double) * (size_t)nseg * nw * nc);
  const size_t o_out = lay.take(o_host ? sizeof(double) * (size_t)nw * nc : 0);
  const size_t o_bval = lay.take(sizeof(double) * (size_t)nw * nblk);
  const size_t o_bpos = lay.take(sizeof(int64_t) * (size_t)nw * nblk);
  const size_t o_best = lay.take(sizeof(double) * MFGP_IVR_MAXW);
  const size_t o_bp = lay.take(sizeof(int64_t) * MFGP_IVR_MAXW);
  if ((rc = ensure_ws(c, lay.end))) return rc;
  char* ws = reinterpret_cast<char*>(c->ws.get());
  int64_t* dcand = cand ? reinterpret_cast<int64_t*>(ws + o_cand) : nullptr;
  if (cand) HIP_TRY(hipMemcpyAsync(dcand, cand, sizeof(int64_t) * nc, hipMemcpyHostToDevice, c->stream));
  const StagedIn sw(w, nw, M, ldw, w_host, ws + o_w);
  HIP_TRY(sw.upload(c->stream));
  const StagedOut so(out, ldo, o_host, ws + o_out, nc);
  double* dbest = want_best ? reinterpret_cast<double*>(ws + o_best) : nullptr;
  int64_t* dbp = want_best ? reinterpret_cast<int64_t*>(ws + o_bp) : nullptr;
  GPDesc d;
  fill_desc(d, m);
  HIP_TRY(launch_ivr(d, dcand, nc, sw.dev, nw, sw.ld, reinterpret_cast<double*>(ws + o_part), so.dev, so.ld,
                     reinterpret_cast<double*>(ws + o_bval), reinterpret_cast<int64_t*>(ws + o_bpos), dbest, dbp,
                     c->stream));
  HIP_TRY(so.copy_back(nc, nw, c->stream));
  if (best) HIP_TRY(hipMemcpyAsync(best, dbest, sizeof(double) * nw, hipMemcpyDeviceToHost, c->stream));
  if (best_pos) HIP_TRY(hipMemcpyAsync(best_pos, dbp, sizeof(int64_t) * nw, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return MFGP_OK;
}

// The posterior covariance applied to grid vectors (mfgp_plan_ivr.hip): per column two
// streamed passes over the resident V and the K** x term, one column after another, so a
// column's bits depend only on the model and that column.
int mfgp_cov_apply(mfgp_model* m, const double* x, int nx, int64_t ldx, double* out, int64_t ldo, int flags) {
  const Entry entry(m);
  int rc = entry.rc;
  if (rc) return rc;
  mfgp_ctx* c = m->ctx;
  const int64_t M = m->M;
  if ((rc = need_f64_grid(m, "mfgp_cov_apply"))) return rc;
  if (nx < 1 || nx > MFGP_IVR_MAXW)
    return set_err(MFGP_ERR_ARG, "mfgp_cov_apply: nx = %d is outside [1, %d]", nx, MFGP_IVR_MAXW);
  if (!x || !out) return set_err(MFGP_ERR_ARG, "mfgp_cov_apply: null vectors / output");
  if (ldx < M)
    return set_err(MFGP_ERR_ARG, "mfgp_cov_apply: ldx = %lld is less than M = %lld", (long long)ldx, (long long)M);
  if (ldo < M)
    return set_err(MFGP_ERR_ARG, "mfgp_cov_apply: ldo = %lld is less than M = %lld", (long long)ldo, (long long)M);
  const bool x_host = !is_device_ptr(x);
  if (const int64_t k = x_host ? finite_rows(x, nx, ldx, M) : -1; k >= 0)
    return set_err(MFGP_ERR_ARG, "mfgp_cov_apply: the vectors must be finite (column %d)", (int)k);
  const bool prior = (flags & MFGP_COV_PRIOR) != 0;
  if (!prior && (rc = ensure_resident_v(m, "mfgp_cov_apply"))) return rc;
  const int64_t N = prior ? 0 : m->NL + m->NH;
  // workspace: [host vectors [nx][M] | out, when it is host memory | the product's scratch]
  const bool o_host = !is_device_ptr(out);
  WsLayout lay;
  const size_t o_x = lay.take(x_host ? sizeof(double) * (size_t)nx * M : 0);
  const size_t o_out = lay.take(o_host ? sizeof(double) * (size_t)nx * M : 0);
  const size_t o_work = lay.take(cov_work_bytes(m, N));
  if ((rc = ensure_ws(c, lay.end))) return rc;
  char* ws = reinterpret_cast<char*>(c->ws.get());
  const StagedIn sx(x, nx, M, ldx, x_host, ws + o_x);
  HIP_TRY(sx.upload(c->stream));
  const StagedOut so(out, ldo, o_host, ws + o_out, M);
  CovWork w;
  if ((rc = cov_work_init(m, ws + o_work, N, w))) return rc;
  for (int k = 0; k < nx; ++k) {
    w.a.x = sx.dev + (int64_t)k * sx.ld;
    w.a.u = so.dev + (int64_t)k * so.ld;
    if ((rc = cov_work_run(m, w, N))) return rc;
  }
  HIP_TRY(so.copy_back(M, nx, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return MFGP_OK;
}

int mfgp_query(mfgp_model* m, const double* Xq, int64_t nq, const double* XL_new, int64_t nl_new,
               const double* XH_new, int64_t nh_new, double* mu, double* var0, double* var, double* cov,
               int64_t ldc) {
  const Entry entry(m);
  int rc = entry.rc;
  if (rc) return rc;
  mfgp_ctx* c = m->ctx;
  if (nq < 0 || nl_new < 0 || nh_new < 0) return set_err(MFGP_ERR_ARG, "mfgp_query: negative count");
  if (nl_new + nh_new > MFGP_LOOK_MAX)
    return set_err(MFGP_ERR_ARG, "mfgp_query: at most %d prospective points per call (got %lld + %lld)", MFGP_LOOK_MAX,
                   (long long)nl_new, (long long)nh_new);
  if (m->kind == MFGP_SF && nl_new != 0)
    return set_err(MFGP_ERR_ARG, "mfgp_query: a single-fidelity model takes its prospective rows in XH_new (nl_new = %lld)",
                   (long long)nl_new);
  if ((nq > 0 && !Xq) || (nl_new > 0 && !XL_new) || (nh_new > 0 && !XH_new))
    return set_err(MFGP_ERR_ARG, "mfgp_query: null points");
  if (cov && ldc < nq)
    return set_err(MFGP_ERR_ARG, "mfgp_query: ldc = %lld is less than nq = %lld", (long long)ldc, (long long)nq);
  const int P = (int)(nl_new + nh_new);
  // host copies of the points: the finite check, the record's key, the upload
  std::vector<double> hq((size_t)2 * nq), hp((size_t)2 * P);
  auto fetch = [&](double* dst, const double* src, int64_t n) -> int {
    if (n <= 0) return MFGP_OK;
    if (is_device_ptr(src)) HIP_TRY(hipMemcpy(dst, src, sizeof(double) * 2 * n, hipMemcpyDeviceToHost));
    else std::memcpy(dst, src, sizeof(double) * 2 * n);
    return MFGP_OK;
  };
  const bool q_dev = nq > 0 && is_device_ptr(Xq);
  if ((rc = fetch(hq.data(), Xq, nq))) return rc;
  if ((rc = fetch(hp.data(), XL_new, nl_new))) return rc;
  if ((rc = fetch(hp.data() + 2 * nl_new, XH_new, nh_new))) return rc;
  if (!all_finite(hq.data(), 2 * nq) || !all_finite(hp.data(), 2 * P))
    return set_err(MFGP_ERR_ARG, "mfgp_query: the points must be finite");
  if ((rc = update_factor(m))) return rc;
  if (nq == 0 && P == 0) return MFGP_OK;
  const int64_t N = m->NL + m->NH;
  if (N > 0 && m->ld > MAX_FULL_CAP + 64)
    return set_err(MFGP_ERR_ARG, "mfgp_query supports a training capacity of at most %lld rows (this model's is %lld)",
                   (long long)MAX_FULL_CAP, (long long)(m->ld - 1));
  LookArgs a{};
  a.X = m->X;
  a.A = m->A;
  a.Linv = m->Linv;
  a.zv = m->zv;
  a.N = N;
  a.NL = m->NL;
  a.ld = m->ld;
  a.h = derive_hyp(m->kind, m->hyp, m->jitter);
  a.P = P;
  if (P > 0) {
    if (!m->look) m->look = new mfgp_look_rec();
    mfgp_look_rec* k = m->look;
    const int64_t wld = std::max<int64_t>(prow_blocks(N) * PRB, PRB);
    if (!k->L22 || !k->pfid) {   // (the pair: a record with one of them allocates again)
      if ((rc = dev_alloc(k->L22, c->stream, sizeof(double) * (2 * TILE + 2 * LOOK_MAX), A_NO_DRAIN))) return rc;
      if ((rc = dev_alloc(k->pfid, c->stream, sizeof(int) * (LOOK_MAX + 1), A_NO_DRAIN))) return rc;
    }
    if (k->wld < wld) {
      k->wld = 0;
      k->valid = false;
      if ((rc = dev_alloc(k->W, c->stream, sizeof(double) * wld * PBM))) return rc;
      k->wld = wld;
    }
    std::vector<double> key(hp);
    for (int i = 0; i < P; ++i) key.push_back(i < nl_new ? 0.0 : 1.0);
    a.W = k->W;
    a.L22 = k->L22;
    a.L22inv = k->L22 + TILE;
    a.ppts = k->L22 + 2 * TILE;
    a.pfid = k->pfid;
    a.status = k->pfid + LOOK_MAX;
    const bool hit = k->valid && k->serial == m->serial && k->P == P && k->key.size() == key.size() &&
                     std::memcmp(k->key.data(), key.data(), sizeof(double) * key.size()) == 0;
    if (!hit) {
      int fid[LOOK_MAX];
      for (int i = 0; i < P; ++i) fid[i] = i < nl_new ? 0 : 1;
      k->valid = false;
      HIP_TRY(hipMemcpyAsync(k->L22 + 2 * TILE, hp.data(), sizeof(double) * 2 * P, hipMemcpyHostToDevice, c->stream));
      HIP_TRY(hipMemcpyAsync(k->pfid, fid, sizeof(int) * P, hipMemcpyHostToDevice, c->stream));
      LookArgs b = a;
      b.vld = k->wld;
      HIP_TRY(launch_look_border(b, c->stream));
      m->cnt[N_LOOK_BORDER] += 1;
      if ((rc = ensure_h_status(c, 1))) return rc;
      HIP_TRY(hipMemcpyAsync(c->h_status, a.status, sizeof(int), hipMemcpyDeviceToHost, c->stream));
      HIP_TRY(hipStreamSynchronize(c->stream));   // (also: hp / fid are read)
      if (c->h_status[0] != INT_MAX)
        return set_err(MFGP_ERR_NOT_PD, "Matrix is not positive definite (look-ahead border, prospective point %d)",
                       c->h_status[0] - 1);
      k->valid = true;
      k->serial = m->serial;
      k->P = P;
      k->key.swap(key);
    }
  }
  if (nq == 0) return MFGP_OK;
  // workspace: [query points | mu | var0 | var (a chunk each) | cov when it goes to the host | scratch tiles]
  const int64_t chunk = cov ? nq : std::min(nq, LOOK_CHUNK);
  const int64_t vld = prow_blocks(N) * PRB + LOOK_MAX;
  const bool cov_host = cov && !is_device_ptr(cov);
  WsLayout lay;
  const size_t o_q = lay.take(sizeof(double) * 2 * chunk);
  const size_t o_out[3] = {lay.take(sizeof(double) * chunk), lay.take(sizeof(double) * chunk),
                           lay.take(sizeof(double) * chunk)};
  const size_t o_cov = lay.take(cov_host ? sizeof(double) * (size_t)nq * nq : 0);
  const size_t o_scr = lay.take(sizeof(double) * (size_t)ntiles_grid(chunk) * vld * PBM);
  if ((rc = ensure_ws(c, lay.end))) return rc;
  char* ws = reinterpret_cast<char*>(c->ws.get());
  double* outs[3] = {mu, var0, var};
  a.scr = reinterpret_cast<double*>(ws + o_scr);
  a.vld = vld;
  a.store_t = cov ? 1 : 0;
  for (int64_t q0 = 0; q0 < nq; q0 += chunk) {
    const int64_t n = std::min(chunk, nq - q0);
    double* dq = reinterpret_cast<double*>(ws + o_q);
    if (q_dev) {
      dq = const_cast<double*>(Xq) + 2 * q0;
    } else {
      HIP_TRY(hipMemcpyAsync(dq, hq.data() + 2 * q0, sizeof(double) * 2 * n, hipMemcpyHostToDevice, c->stream));
    }
    a.pts = dq;
    a.M = n;
    double* kout[3];
    bool khost[3];
    for (int i = 0; i < 3; ++i) {
      khost[i] = outs[i] && !is_device_ptr(outs[i]);
      kout[i] = !outs[i] ? nullptr
                         : (khost[i] ? reinterpret_cast<double*>(ws + o_out[i]) : outs[i] + q0);
    }
    a.mu = kout[0];
    a.var0 = kout[1];
    a.var = kout[2];
    HIP_TRY(launch_look_query(a, c->stream));
    m->cnt[N_LOOK_QUERY] += 1;
    if (cov) {
      // the scratch as a V of N + P rows over the query points: k_cov_block's GEMM
      GPDesc d{};
      d.V = a.scr;
      d.vld = vld;
      d.grid = dq;
      d.M = n;
      d.N = N + P;
      d.hp = a.h;
      const StagedOut so(cov, ldc, cov_host, ws + o_cov, nq);
      HIP_TRY(launch_cov_block(d, nullptr, n, nullptr, n, so.dev, so.ld, d.N == 0 ? 1 : 0, c->stream));
      HIP_TRY(so.copy_back(nq, nq, c->stream));
    }
    for (int i = 0; i < 3; ++i)
      if (khost[i])
        HIP_TRY(hipMemcpyAsync(outs[i] + q0, kout[i], sizeof(double) * n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));   // the chunk's staging is reused by the next
  }
  return MFGP_OK;
}

// Pathwise samples (mfgp_sample.hip). The axis factor: a diagonally pivoted Cholesky
// of the unit-diagonal axis Gram exp(-(a_i / l - a_j / l)^2 / 2), stopped when the
// largest remaining diagonal entry is <= 2^-50. cols: rank columns of n entries each
// (column k = the k-th pivot step; rows are not permuted, so cols cols^T = K up to the
// positive semi-definite remainder).
constexpr double SAMPLE_PIVOT_STOP = 0x1p-50;
constexpr int SAMPLE_AXIS_MAX = 4096;              // lattice axis length the sampler serves
constexpr size_t SAMPLE_T_MAX = size_t(1) << 30;   // bytes of the chunk's Ax Z scratch

static int axis_factor(const double* axis, int n, double l, std::vector<double>& cols) {
  cols.clear();
  std::vector<double> t((size_t)n), d((size_t)n, 1.0);
  std::vector<char> used((size_t)n, 0);
  for (int i = 0; i < n; ++i) t[i] = axis[i] / l;
  int rank = 0;
  for (int k = 0; k < n; ++k) {
    int p = -1;
    double best = SAMPLE_PIVOT_STOP;
    for (int i = 0; i < n; ++i)
      if (!used[i] && d[i] > best) {
        best = d[i];
        p = i;
      }
    if (p < 0) break;
    const double piv = std::sqrt(best);
    cols.resize((size_t)(k + 1) * n);
    double* c = cols.data() + (size_t)k * n;
    for (int i = 0; i < n; ++i) {
      if (used[i]) {
        c[i] = 0.0;
        continue;
      }
      if (i == p) {
        c[i] = piv;
        continue;
      }
      const double dx = t[i] - t[p];
      double v = std::exp(-0.5 * (dx * dx));
      for (int j = 0; j < k; ++j) v -= cols[(size_t)j * n + i] * cols[(size_t)j * n + p];
      c[i] = v / piv;
      d[i] -= c[i] * c[i];
    }
    used[p] = 1;
    d[p] = 0.0;
    rank = k + 1;
  }
  return rank;
}

int mfgp_sample_axis_factor(const double* axis, int n, double lengthscale, double* A, int* rank) {
  if (n < 0 || (n > 0 && (!axis || !A)) || !rank)
    return set_err(MFGP_ERR_ARG, "mfgp_sample_axis_factor: null pointer or negative n");
  if (!(lengthscale > 0.0) || !std::isfinite(lengthscale))
    return set_err(MFGP_ERR_ARG, "mfgp_sample_axis_factor: the length scale must be positive and finite");
  if (!all_finite(axis, n)) return set_err(MFGP_ERR_ARG, "mfgp_sample_axis_factor: the axis values must be finite");
  std::vector<double> cols;
  const int r = axis_factor(axis, n, lengthscale, cols);
  for (int i = 0; i < n; ++i)
    for (int k = 0; k < n; ++k) A[(size_t)i * n + k] = k < r ? cols[(size_t)k * n + i] : 0.0;
  *rank = r;
  return MFGP_OK;
}

// The checks and the record every sample entry point shares, without any launch: the
// model serves samples (fp64, a lattice grid within the sampler's sizes) and its sample
// record holds the axis factors of the current serial.
static int sample_record(mfgp_model* m, const char* who) {
  if (const int rc = need_f64_grid(m, who)) return rc;
  const GridLattice& L = m->lat;
  if (L.nx <= 0 || L.ny <= 0)
    return set_err(MFGP_ERR_NO_LATTICE, "%s: the grid is not a lattice of two axes", who);
  if (L.nx > SAMPLE_AXIS_MAX || L.ny > SAMPLE_AXIS_MAX)
    return set_err(MFGP_ERR_ARG, "%s: lattice axes of at most %d values are supported (this grid's: %d x %d)", who,
                   SAMPLE_AXIS_MAX, L.nx, L.ny);
  if (!m->samp) m->samp = new mfgp_sample_rec();
  mfgp_sample_rec* k = m->samp;
  if (k->valid && k->serial == m->serial) return MFGP_OK;
  mfgp_ctx* c = m->ctx;
  k->valid = false;
  HIP_TRY(hipStreamSynchronize(c->stream));
  std::vector<double> ax((size_t)L.nx), ay((size_t)L.ny);
  HIP_TRY(hipMemcpy2D(ax.data(), sizeof(double), m->grid, sizeof(double) * 2 * L.sx, sizeof(double), L.nx,
                      hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy2D(ay.data(), sizeof(double), m->grid + 1, sizeof(double) * 2 * L.sy, sizeof(double), L.ny,
                      hipMemcpyDeviceToHost));
  const Hyp h = derive_hyp(m->kind, m->hyp, m->jitter);
  const int fields = m->kind == MFGP_SF ? 1 : 2;
  std::vector<double> host;
  for (int f = 0; f < fields; ++f) {
    const double l = f ? h.lH : h.lL;
    if (!(l > 0.0) || !std::isfinite(l)) return set_err(MFGP_ERR_ARG, "%s: the length scales must be positive and finite", who);
    std::vector<double> cx, cy;
    k->rx[f] = axis_factor(ax.data(), L.nx, l, cx);
    k->ry[f] = axis_factor(ay.data(), L.ny, l, cy);
    k->off_ax[f] = host.size();   // Ax [nx][rx] row-major
    host.resize(host.size() + (size_t)L.nx * k->rx[f]);
    for (int i = 0; i < L.nx; ++i)
      for (int a = 0; a < k->rx[f]; ++a) host[k->off_ax[f] + (size_t)i * k->rx[f] + a] = cx[(size_t)a * L.nx + i];
    k->off_ay[f] = host.size();   // AyT [ry][ny]: the columns as they are
    host.insert(host.end(), cy.begin(), cy.end());
  }
  if (fields == 1) k->rx[1] = k->ry[1] = 0;
  if (host.size() > k->fac_n) {
    k->fac_n = 0;
    if (const int rc = dev_alloc(k->fac, c->stream, sizeof(double) * host.size(), A_NO_DRAIN)) return rc;
    k->fac_n = host.size();
  }
  HIP_TRY(hipMemcpy(k->fac, host.data(), sizeof(double) * host.size(), hipMemcpyHostToDevice));
  k->fields = fields;
  k->nx = L.nx;
  k->ny = L.ny;
  k->serial = m->serial;
  k->valid = true;
  return MFGP_OK;
}

static int64_t sample_nz(const mfgp_model* m, bool prior) {
  const mfgp_sample_rec* k = m->samp;
  return (int64_t)k->rx[0] * k->ry[0] + (int64_t)k->rx[1] * k->ry[1] + (prior ? 0 : m->NL + m->NH);
}

// The lattice indices of the N training rows into the record (host search by exact
// equality on the axis values, as the lattice step's tables do on the device).
static int sample_lidx(mfgp_model* m, const char* who) {
  mfgp_sample_rec* k = m->samp;
  mfgp_ctx* c = m->ctx;
  const int64_t N = m->NL + m->NH;
  const GridLattice& L = m->lat;
  if (!(k->lidx_valid && k->lidx_serial == m->serial)) {
    k->lidx_valid = false;
    HIP_TRY(hipStreamSynchronize(c->stream));
    std::vector<double> ax((size_t)L.nx), ay((size_t)L.ny), X((size_t)2 * N);
    HIP_TRY(hipMemcpy2D(ax.data(), sizeof(double), m->grid, sizeof(double) * 2 * L.sx, sizeof(double), L.nx,
                        hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy2D(ay.data(), sizeof(double), m->grid + 1, sizeof(double) * 2 * L.sy, sizeof(double), L.ny,
                        hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(X.data(), m->X, sizeof(double) * 2 * N, hipMemcpyDeviceToHost));
    auto find = [](const std::vector<double>& a, double v) -> int {   // a strictly monotone, either way
      const bool up = a.size() < 2 || a[1] > a[0];
      int64_t lo = 0, hi = (int64_t)a.size() - 1;
      while (lo <= hi) {
        const int64_t mid = (lo + hi) / 2;
        if (a[mid] == v) return (int)mid;
        if ((a[mid] < v) == up) lo = mid + 1;
        else hi = mid - 1;
      }
      return -1;
    };
    std::vector<int> li((size_t)N);
    k->off_row = -1;
    for (int64_t i = 0; i < N; ++i) {
      const int px = find(ax, X[2 * i]), py = find(ay, X[2 * i + 1]);
      li[i] = (px >= 0 && py >= 0) ? (px | (py << 16)) : -1;
      if (li[i] < 0 && k->off_row < 0) k->off_row = i;
    }
    if (k->lidx_cap < N) {
      k->lidx_cap = 0;
      if (const int rc = dev_alloc(k->lidx, c->stream, sizeof(int) * round_up(N, 1024), A_NO_DRAIN)) return rc;
      k->lidx_cap = round_up(N, 1024);
    }
    HIP_TRY(hipMemcpy(k->lidx, li.data(), sizeof(int) * N, hipMemcpyHostToDevice));
    k->lidx_serial = m->serial;
    k->lidx_valid = true;
  }
  if (k->off_row >= 0)
    return set_err(MFGP_ERR_NO_LATTICE, "%s: training row %lld is not a cell of the grid's lattice", who,
                   (long long)k->off_row);
  return MFGP_OK;
}

int mfgp_sample_dims(mfgp_model* m, int64_t* dims, int n, int flags) {
  const Entry entry(m);
  int rc = entry.rc;
  if (rc) return rc;
  if (n < 0 || (n > 0 && !dims)) return set_err(MFGP_ERR_ARG, "mfgp_sample_dims: null dims");
  const bool prior = (flags & MFGP_SAMPLE_PRIOR) != 0;
  if ((rc = sample_record(m, "mfgp_sample_dims"))) return rc;
  if (!prior && (rc = ensure_resident_v(m, "mfgp_sample_dims"))) return rc;
  const mfgp_sample_rec* k = m->samp;
  const int64_t v[8] = {sample_nz(m, prior), m->M, prior ? 0 : m->NL + m->NH, k->fields,
                        k->rx[0], k->ry[0], k->rx[1], k->ry[1]};
  for (int i = 0; i < n && i < 8; ++i) dims[i] = v[i];
  return MFGP_OK;
}

int mfgp_sample_posterior(mfgp_model* m, const double* normals, int64_t S, int64_t ldz, double* out, int64_t ldo,
                          int flags) {
  const char* who = "mfgp_sample_posterior";
  const Entry entry(m);
  int rc = entry.rc;
  if (rc) return rc;
  mfgp_ctx* c = m->ctx;
  const bool prior = (flags & MFGP_SAMPLE_PRIOR) != 0;
  if (S < 0) return set_err(MFGP_ERR_ARG, "%s: negative sample count", who);
  if (m->dtype == MFGP_F64 && m->M > 0 && ldo < m->M)
    return set_err(MFGP_ERR_ARG, "%s: ldo = %lld is less than M = %lld", who, (long long)ldo, (long long)m->M);
  if ((rc = sample_record(m, who))) return rc;
  const mfgp_sample_rec* k = m->samp;
  const int64_t N = prior ? 0 : m->NL + m->NH, M = m->M;
  const int64_t nz = sample_nz(m, prior);
  if (ldz < nz) return set_err(MFGP_ERR_ARG, "%s: ldz = %lld is less than nz = %lld", who, (long long)ldz, (long long)nz);
  if (S > 0 && (!out || (nz > 0 && !normals))) return set_err(MFGP_ERR_ARG, "%s: null normals / output", who);
  const bool z_dev = S > 0 && nz > 0 && is_device_ptr(normals);
  const bool o_dev = S > 0 && is_device_ptr(out);
  const bool z_host = !z_dev && nz > 0;   // the normals are staged chunk by chunk
  if (z_host && finite_rows(normals, S, ldz, nz) >= 0)
    return set_err(MFGP_ERR_ARG, "%s: the normals must be finite", who);
  const int64_t tw = std::max(std::max(k->ry[0], k->ry[1]), 1);
  const size_t t_bytes = sizeof(double) * (size_t)SAMPLE_CHUNK * k->fields * k->nx * tw;
  if (t_bytes > SAMPLE_T_MAX)
    return set_err(MFGP_ERR_ARG, "%s: the axis factors' ranks (%d, %d) on %d x %d axes need more than %zu bytes of scratch",
                   who, k->ry[0], k->ry[1], k->nx, k->ny, SAMPLE_T_MAX);
  if (S == 0) return MFGP_OK;
  if (N > 0) {
    if ((rc = ensure_resident_v(m, who))) return rc;
    if ((rc = sample_lidx(m, who))) return rc;
    if (m->ld > MAX_FULL_CAP + 64)
      return set_err(MFGP_ERR_ARG, "%s supports a training capacity of at most %lld rows (this model's is %lld)", who,
                     (long long)MAX_FULL_CAP, (long long)(m->ld - 1));
  }
  // workspace: [T | R | W | the chunk's normals (host normals) | the chunk's samples (host output)]
  const int64_t wld = std::max<int64_t>(prow_blocks(N) * PRB, PRB);
  WsLayout lay;
  const size_t o_t = lay.take(t_bytes), o_r = lay.take(sizeof(double) * wld * PBM);
  const size_t o_w = lay.take(sizeof(double) * wld * PBM);
  const size_t o_z = lay.take(z_dev ? 0 : sizeof(double) * (size_t)SAMPLE_CHUNK * std::max<int64_t>(nz, 1));
  const size_t o_o = lay.take(o_dev ? 0 : sizeof(double) * (size_t)SAMPLE_CHUNK * M);
  if ((rc = ensure_ws(c, lay.end))) return rc;
  char* ws = reinterpret_cast<char*>(c->ws.get());
  const Hyp h = derive_hyp(m->kind, m->hyp, m->jitter);
  const GridLattice& L = m->lat;
  SampleArgs a{};
  a.M = M;
  a.fields = k->fields;
  a.nx = L.nx;
  a.ny = L.ny;
  a.sx = L.sx;
  a.sy = L.sy;
  a.zoff[0] = 0;
  a.zoff[1] = (int64_t)k->rx[0] * k->ry[0];
  a.zoff[2] = a.zoff[1] + (int64_t)k->rx[1] * k->ry[1];
  for (int f = 0; f < 2; ++f) {
    a.rx[f] = k->rx[f];
    a.ry[f] = k->ry[f];
    a.Ax[f] = k->fac + k->off_ax[f];
    a.AyT[f] = k->fac + k->off_ay[f];
  }
  a.T = reinterpret_cast<double*>(ws + o_t);
  a.tw = tw;
  a.cL = std::sqrt(h.sL);
  a.cH[0] = m->kind == MFGP_SF ? std::sqrt(h.sL) : h.rho * std::sqrt(h.sL);
  a.cH[1] = std::sqrt(h.sH);
  a.mean = prior ? 0.0 : h.meanH;
  a.meanL = h.meanL;
  a.meanH = h.meanH;
  a.sdL = std::sqrt(h.noiseL + h.jitter);
  a.sdH = std::sqrt(h.noiseH + h.jitter);
  a.y = m->y;
  a.lidx = k->lidx;
  a.N = N;
  a.NL = m->NL;
  a.R = reinterpret_cast<double*>(ws + o_r);
  a.W = reinterpret_cast<double*>(ws + o_w);
  a.wld = wld;
  a.A = m->A;
  a.Linv = m->Linv;
  a.ld = m->ld;
  a.V = static_cast<const double*>(m->V.get());
  a.vld = m->vld;
  for (int64_t s0 = 0; s0 < S; s0 += SAMPLE_CHUNK) {
    const int64_t sc = std::min<int64_t>(SAMPLE_CHUNK, S - s0);
    a.Sc = (int)sc;
    const StagedIn sz(normals ? normals + s0 * ldz : nullptr, sc, nz, ldz, z_host, ws + o_z);
    HIP_TRY(sz.upload(c->stream));
    a.Z = sz.dev;
    a.ldz = sz.ld;
    const StagedOut so(out + s0 * ldo, ldo, !o_dev, ws + o_o, M);
    a.out = so.dev;
    a.ldo = so.ld;
    HIP_TRY(launch_sample_prior(a, c->stream));
    if (N > 0) {
      HIP_TRY(launch_sample_resid(a, c->stream));
      HIP_TRY(launch_sample_solve(a, c->stream));
      m->cnt[N_SAMPLE_SOLVE] += 1;
      HIP_TRY(launch_sample_gemm(a, c->stream));
      m->cnt[N_SAMPLE_GEMM] += 1;
    }
    HIP_TRY(so.copy_back(M, sc, c->stream));
    if (!o_dev || z_host) HIP_TRY(hipStreamSynchronize(c->stream));   // the staging is reused by the next chunk
  }
  HIP_TRY(hipStreamSynchronize(c->stream));
  return MFGP_OK;
}

}  // extern "C"
