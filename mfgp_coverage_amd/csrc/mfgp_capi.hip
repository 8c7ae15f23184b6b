// C ABI of libmfgp_hip.so (declared in include/mfgp_hip.h).
//
// Host-side state management for the GP posterior engine: contexts (one HIP
// stream + workspace each), models (device-resident training set, factor and
// grid) and their state helpers, set / append / truncate / predict and the views,
// timing, statistics and error reporting. The batched update+predict driver is
// mfgp_step.hip; mfgp_host.h lists the other host files.
// Mirrors the reference methods cited in include/mfgp_hip.h.
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>

#include "mfgp_host.h"

using namespace mfgp;
using namespace mfgp_host;

namespace {
thread_local std::string g_err;
std::atomic<uint64_t> g_serial{0};
}  // namespace

namespace mfgp_host __attribute__((visibility("hidden"))) {

mfgp_own::Live live_dev, live_pin;

int set_err(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

void bump_serial(mfgp_model* m) { m->serial = g_serial.fetch_add(1, std::memory_order_relaxed) + 1; }

Hyp derive_hyp(int kind, const double* hyp, double jitter) {
  Hyp h{};
  h.kind = kind;
  h.jitter = jitter;
  if (kind == MFGP_SF) {
    // [mu, s^2, L, noise]  (gp:75-76, gp:132, gp:248-249)
    h.sL = std::exp(hyp[1]);
    h.lL = std::exp(hyp[2]);
    h.sH = h.sL;
    h.lH = h.lL;
    h.rho = 1.0;
    h.rho2 = 1.0;
    h.noiseL = h.noiseH = std::exp(hyp[3]);
    h.meanL = h.meanH = std::exp(hyp[0]);
    h.kss = h.sL;  // kernel(X*,X*) diagonal = s * exp(0)
  } else {
    // [mu_lo, s^2_lo, L_lo, mu_hi, s^2_hi, L_hi, rho, noise_lo, noise_hi]  (gp:510-514, 414-416)
    h.sL = std::exp(hyp[1]);
    h.lL = std::exp(hyp[2]);
    h.sH = std::exp(hyp[4]);
    h.lH = std::exp(hyp[5]);
    h.rho = std::exp(hyp[6]);
    h.rho2 = h.rho * h.rho;
    h.noiseL = std::exp(hyp[7]);
    h.noiseH = std::exp(hyp[8]);
    h.meanL = std::exp(hyp[0]);
    h.meanH = h.rho * h.meanL + std::exp(hyp[3]);
    h.kss = h.rho2 * h.sL + h.sH;  // gp:435-436 diagonal
  }
  return h;
}

static int drain_timing(mfgp_ctx* c) {
  for (auto& p : c->pending) {
    HIP_TRY(hipEventSynchronize(p.b));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, p.a, p.b));
    if (p.kind == 0) {
      c->t_predict += ms;
      c->n_predict += 1;
    } else {
      c->t_factor += ms;
      c->n_factor += 1;
    }
    c->pool.push_back(p.a);
    c->pool.push_back(p.b);
  }
  c->pending.clear();
  return MFGP_OK;
}

int ensure_h_status(mfgp_ctx* c, size_t n) {
  if (sizeof(int) * n <= c->h_status.bytes()) return MFGP_OK;
  HIP_TRY(hipStreamSynchronize(c->stream));
  return pin_alloc(c->h_status, sizeof(int) * std::max<size_t>(n, 64), hipHostMallocDefault);
}

int ensure_ws(mfgp_ctx* c, size_t bytes) {
  if (bytes <= c->ws.bytes()) return MFGP_OK;
  return dev_alloc(c->ws, c->stream, std::max(bytes, c->ws.bytes() + c->ws.bytes() / 2));
}

// Grow the training capacity of m to hold `need` rows. Keeps X / y and, when
// the factor is current for some rows, A / Linv / zv too (copied into the new
// leading dimension), so a growing GP stays on the incremental path.
int ensure_cap(mfgp_model* m, int64_t need) {
  if (need <= m->cap && m->A) return MFGP_OK;
  mfgp_ctx* c = m->ctx;
  int64_t cap = std::max<int64_t>({need, m->cap + m->cap / 2, 63});
  // the full predict (k_predict) addresses A through a 32-bit buffer descriptor:
  // ld <= 16383, i.e. a capacity of at most MAX_FULL_CAP rows; 1.5x growth stops there
  if (cap > MAX_FULL_CAP && need <= MAX_FULL_CAP) cap = MAX_FULL_CAP;
  int64_t ld = round_up(cap + 1, NB);
  cap = ld - 1;
  // the new buffers in local owners: a failure anywhere before the swap below frees them
  // and leaves the model exactly as it was
  Dev<double> X, y, A, Li, zv, isc, F, tab;
  Dev<float> Ff;
  Dev<int> lidx;
  hipStream_t s = c->stream;
  int rc;
  HIP_TRY(hipStreamSynchronize(s));
  if ((rc = dev_alloc(X, s, sizeof(double) * 2 * cap, A_NO_DRAIN))) return rc;
  if ((rc = dev_alloc(y, s, sizeof(double) * cap, A_NO_DRAIN))) return rc;
  if ((rc = dev_alloc(zv, s, sizeof(double) * cap, A_NO_DRAIN))) return rc;
  if ((rc = dev_alloc(isc, s, sizeof(double) * inc_scratch_doubles(cap), A_NO_DRAIN))) return rc;
  // producer ready flags start below every epoch (epochs are never 0)
  HIP_TRY(hipMemsetAsync(isc + inc_pflag_offset(cap), 0, sizeof(unsigned) * inc_pflag_count(cap), s));
  if ((rc = dev_alloc(A, s, sizeof(double) * ld * ld, A_NO_DRAIN))) return rc;
  if ((rc = dev_alloc(Li, s, sizeof(double) * (ld / NB) * TILE, A_NO_DRAIN))) return rc;
  const int64_t n = m->NL + m->NH;
  if (n > 0) {
    HIP_TRY(hipMemcpyAsync(X, m->X, sizeof(double) * 2 * n, hipMemcpyDeviceToDevice, s));
    HIP_TRY(hipMemcpyAsync(y, m->y, sizeof(double) * n, hipMemcpyDeviceToDevice, s));
  }
  const bool keep = m->A && m->st.factored && m->st.ablk > 0;
  if (keep) {
    HIP_TRY(hipMemcpy2DAsync(A, sizeof(double) * ld, m->A, sizeof(double) * m->ld, sizeof(double) * m->ld, m->ld,
                             hipMemcpyDeviceToDevice, s));
    HIP_TRY(hipMemcpyAsync(Li, m->Linv, sizeof(double) * (m->ld / NB) * TILE, hipMemcpyDeviceToDevice, s));
    HIP_TRY(hipMemcpyAsync(zv, m->zv, sizeof(double) * m->cap, hipMemcpyDeviceToDevice, s));
  }
  // the lattice step's F and tables move to the new leading dimension too
  const int64_t F_n = m->st.F.n, tab_n = m->st.tab.n;   // (whatever their generation: the rows stay what they were)
  if (keep && m->F && F_n > 0) {
    if ((rc = dev_alloc(F, s, sizeof(double) * fblk_size(ld), A_ZERO | A_NO_DRAIN))) return rc;
    for (int64_t jb = 0; 64 * jb < F_n; ++jb)   // each column block's rows [64 jb, F_n)
      HIP_TRY(hipMemcpyAsync(F + fblk_off(jb, ld), m->F + fblk_off(jb, m->F_ld),
                             sizeof(double) * 64 * (F_n - 64 * jb), hipMemcpyDeviceToDevice, s));
    if (m->Ff) {   // (MFGP_F32: the rows past the build live in Ff only)
      if ((rc = dev_alloc(Ff, s, sizeof(float) * fblk_size(ld), A_ZERO | A_NO_DRAIN))) return rc;
      for (int64_t jb = 0; 64 * jb < F_n; ++jb)
        HIP_TRY(hipMemcpyAsync(Ff + fblk_off(jb, ld), m->Ff + fblk_off(jb, m->F_ld),
                               sizeof(float) * 64 * (F_n - 64 * jb), hipMemcpyDeviceToDevice, s));
    }
  }
  if (m->tab && tab_n > 0) {
    if ((rc = dev_alloc(tab, s, sizeof(double) * 4 * ld * m->tabw, A_ZERO | A_NO_DRAIN))) return rc;
    for (int t = 0; t < 4; ++t)
      HIP_TRY(hipMemcpyAsync(tab + (size_t)t * ld * m->tabw, m->tab + (size_t)t * m->tab_ld * m->tabw,
                             sizeof(double) * tab_n * m->tabw, hipMemcpyDeviceToDevice, s));
    if ((rc = dev_alloc(lidx, s, sizeof(int) * ld, A_NO_DRAIN))) return rc;
    HIP_TRY(hipMemcpyAsync(lidx, m->lidx, sizeof(int) * tab_n, hipMemcpyDeviceToDevice, s));
  }
  HIP_TRY(hipStreamSynchronize(s));
  // the commit: nothing below fails; the locals leave with the old buffers and free them
  m->lidx.swap(lidx);
  m->F.swap(F);
  m->Ff.swap(Ff);
  m->F_ld = m->F ? ld : 0;
  if (!m->F) m->st.f_reallocated();
  m->tab.swap(tab);
  m->tab_ld = m->tab ? ld : 0;
  if (!m->tab) m->st.tab_reallocated();
  m->X.swap(X);
  m->y.swap(y);
  m->A.swap(A);
  m->Linv.swap(Li);
  m->zv.swap(zv);
  m->iscr.swap(isc);
  m->st.compact_rows_reallocated();
  m->cap = cap;
  m->ld = ld;
  if (!keep) {
    m->st.factor_lost(FactorLost::Reallocated);
    m->st.v_dropped();
  }
  return MFGP_OK;
}

// Resident V for the current capacity and grid (contents kept when it fits).
static size_t v_elem(const mfgp_model* m) { return m->dtype == MFGP_F32 ? sizeof(float) : sizeof(double); }

int ensure_v(mfgp_model* m) {
  const int64_t vld = round_up(m->cap, PRB);
  const int64_t tiles = ntiles_grid(m->M);
  if (m->V && m->tred && m->vld == vld && m->vtiles >= tiles) return MFGP_OK;
  hipStream_t s = m->ctx->stream;
  const size_t es = v_elem(m);
  int rc;
  Dev<void> V;   // committed once the valid rows are in it: until then the model keeps its own
  if ((rc = dev_alloc(V, s, es * (size_t)tiles * vld * PBM, A_NO_DRAIN))) return rc;
  const bool moved = m->V && m->st.v_n > 0 && m->vtiles >= tiles && m->vld >= m->st.v_n;
  if (moved)   // capacity grew: move the valid rows of every tile to the new row stride
    HIP_TRY(hipMemcpy2DAsync(V, es * vld * PBM, m->V, es * m->vld * PBM, es * m->st.v_n * PBM, tiles,
                             hipMemcpyDeviceToDevice, s));
  HIP_TRY(hipStreamSynchronize(s));
  if (!moved) m->st.v_dropped();
  m->V.swap(V);
  V.reset();
  m->vld = vld;
  if (tiles > m->vtiles || !m->tred) {
    // [arrival counter | (max, argmax) per 64-cell tile (k_predict) or per 32-cell
    // wave group (one-pass predicts)]; the counter is zero between launches (the
    // last arriver of each launch resets it)
    m->tred_n = 0;
    if ((rc = dev_alloc(m->tred, s, sizeof(double) * (4 * tiles + 1), A_ZERO))) return rc;
    HIP_TRY(hipStreamSynchronize(s));
    m->tred_n = 4 * tiles + 1;
  }
  m->vtiles = tiles;
  return MFGP_OK;
}

int check_model(const mfgp_model* m) {
  if (!m || !m->ctx) return set_err(MFGP_ERR_ARG, "null model");
  return MFGP_OK;
}

// A descriptor of m's state: everything a step does not set stays zero / null, but
// one row split, eight new-row slots and no split-K.
void fill_desc(GPDesc& d, mfgp_model* m) {
  d = GPDesc{};
  d.X = m->X;
  d.y = m->y;
  d.A = m->A;
  d.Linv = m->Linv;
  d.grid = m->grid;
  d.lat = m->lat;
  d.V = m->dtype == MFGP_F64 ? static_cast<double*>(m->V.get()) : nullptr;
  d.Vf = m->dtype == MFGP_F32 ? static_cast<float*>(m->V.get()) : nullptr;
  d.vf32 = m->dtype == MFGP_F32 ? 1 : 0;
  d.zv = m->zv;
  d.iscr = m->iscr;
  d.l21c = m->iscr ? m->iscr + inc_l21c_offset(m->cap) : nullptr;
  d.l22r = m->iscr ? m->iscr + inc_l22r_offset(m->cap) : nullptr;
  d.pflag = m->iscr ? reinterpret_cast<unsigned*>(m->iscr + inc_pflag_offset(m->cap)) : nullptr;
  d.tred = m->tred;
  d.gate = m->gate_dev;
  d.status = m->status;
  d.rsplit = 1;
  d.ld = m->ld;
  d.N = m->NL + m->NH;
  d.NL = m->NL;
  d.M = m->M;
  d.vld = m->vld;
  d.ablk = m->st.ablk;
  d.ka = 8;
  d.ksplit = 1;
  d.hf = derive_hyp(m->kind, m->hyp, m->jitter);
  d.hp = d.hf;
}

// ---- resident posterior (two buffers, tagged with the rows and generation) ----
static int ensure_res(mfgp_model* m) {
  if (m->res && m->res_M >= m->M) return MFGP_OK;
  m->res_M = 0;
  m->st.res_reallocated();
  if (const int rc = dev_alloc(m->res, m->ctx->stream, sizeof(double) * 4 * (size_t)m->M)) return rc;
  m->res_M = m->M;
  return MFGP_OK;
}
double* res_mu(mfgp_model* m, int b) { return m->res + (size_t)b * 2 * m->res_M; }
double* res_var(mfgp_model* m, int b) { return m->res + (size_t)b * 2 * m->res_M + m->res_M; }
// the buffer holding the posterior of the n leading rows (-1: none)
int res_find(const mfgp_model* m, int64_t n) { return m->res ? m->st.res_find(n) : -1; }
// Point a predict descriptor's resident outputs at a buffer (incremental mode): not
// `keep`, else the least recently written; returns the buffer (-1: none). Tag it once
// the launch is enqueued (predict_enqueued).
int set_res_out(mfgp_model* m, GPDesc& d, int keep) {
  if (!m->ctx->incremental || m->M <= 0 || ensure_res(m) != MFGP_OK) return -1;
  const int b = m->st.res_out(keep);
  d.rmu = res_mu(m, b);
  d.rvar = res_var(m, b);
  return b;
}

// F, the tables, w and the flags at the model's leading dimension (contents kept
// across capacity growth: ensure_cap moves them)
int ensure_lat(mfgp_model* m, int64_t tiles, int ksplit, int ka, int64_t nzu) {
  hipStream_t s = m->ctx->stream;
  const int64_t ld = m->ld, tabw = lat_tabw(m);
  const bool ff = m->dtype == MFGP_F32;   // (F streamed in fp32: DESIGN.md section 2.3)
  int rc;
  // Each group: the extent it is keyed by reset with the buffers (free-then-allocate: F, the
  // tables and their kin never exist twice), set again once all of the group are there. A
  // refused allocation leaves the group empty behind an extent that makes the next call
  // allocate again.
  if (!m->F || m->F_ld != ld || (ff && !m->Ff)) {
    m->F_ld = 0;
    m->st.f_reallocated();
    if ((rc = dev_alloc(m->F, s, sizeof(double) * fblk_size(ld), A_ZERO))) return rc;   // F's upper triangle stays zero
    m->Ff.reset();
    if (ff && (rc = dev_alloc(m->Ff, s, sizeof(float) * fblk_size(ld), A_ZERO))) return rc;
    m->F_ld = ld;
  }
  if (!m->tab || m->tab_ld != ld || m->tabw != tabw) {
    m->tab_ld = m->tabw = 0;
    m->st.tab_reallocated();
    if ((rc = dev_alloc(m->tab, s, sizeof(double) * 4 * ld * tabw, A_ZERO))) return rc;
    if ((rc = dev_alloc(m->lidx, s, sizeof(int) * ld))) return rc;
    m->tab_ld = ld;
    m->tabw = tabw;
  }
  if (!m->wv || m->wv_ld != ld) {
    m->wv_ld = 0;
    if ((rc = dev_alloc(m->wv, s, sizeof(double) * ld * KINC, A_ZERO))) return rc;
    if ((rc = dev_alloc(m->wflag, s, sizeof(unsigned) * (ld / 64 + 2), A_ZERO))) return rc;   // below every epoch
    if ((rc = dev_alloc(m->wcnt, s, sizeof(unsigned) * 2 * (ld / 64 + 2), A_ZERO))) return rc;
    if ((rc = dev_alloc(m->wpart, s, sizeof(double) * 1024 * (LAT_WU_MAX + ld / 64 + 1)))) return rc;
    m->wv_ld = ld;
  }
  if (m->gcnt_n != tiles) {
    // [tiles] arrival counters of the splits | [tiles] flags (the epoch once all arrived)
    m->gcnt_n = 0;
    if ((rc = dev_alloc(m->gcnt, s, sizeof(unsigned) * 2 * tiles, A_ZERO))) return rc;   // flags below every epoch
    m->gcnt_n = tiles;
  }
  // the fused var max / argmax: one (max, argmax) slot per GEMM workgroup
  if (m->tred && 2 * tiles * ksplit + 1 > m->tred_n) {
    const int64_t nd = 2 * tiles * ksplit + 1;
    m->tred_n = 0;   // (a refused tred: ensure_v allocates it again)
    if ((rc = dev_alloc(m->tred, s, sizeof(double) * nd, A_ZERO))) return rc;
    m->tred_n = nd;
  }
  if (!m->axt || m->axt_w != tabw) {
    m->axt_w = 0;
    if ((rc = dev_alloc(m->axt, s, sizeof(double) * 4 * (tabw + 1) * tabw, A_2M))) return rc;
    m->axt_w = tabw;
    m->st.axt_reallocated();
  }
  // Z rows: per part the lattice y-rows (padded to ZKS), then one per training row
  // that could lie off the lattice; zeros where never written (padding rows)
  const int64_t zrows = round_up(m->lat.ny, ZKS) + ld;
  if (!m->zb || m->zb_rows != zrows || m->zb_w != tabw || m->zb_ka < ka) {
    m->zb_rows = m->zb_w = 0;
    m->zb_ka = 0;
    if ((rc = dev_alloc(m->zb, s, sizeof(double) * 2 * zrows * tabw * ka, A_ZERO))) return rc;
    if ((rc = dev_alloc(m->zvl, s, sizeof(int) * 2 * (zrows + 1), A_ZERO))) return rc;
    m->zb_rows = zrows;
    m->zb_w = tabw;
    m->zb_ka = ka;
  }
  // (the member lists' extent is the owner's own: empty reads as 0 bytes)
  if ((int64_t)m->csr.bytes() < csr_bytes(tabw, ld) && (rc = dev_alloc(m->csr, s, csr_bytes(tabw, ld), A_2M))) return rc;
  if (!m->ldone && (rc = dev_alloc(m->ldone, s, sizeof(unsigned) * 4, A_ZERO))) return rc;   // no arrivals; flags below every epoch
  if (m->zflag_n < nzu + 2) {
    m->zflag_n = 0;
    if ((rc = dev_alloc(m->zflag, s, sizeof(unsigned) * (nzu + 2), A_ZERO))) return rc;   // below every epoch
    m->zflag_n = (nzu + 2);
  }
  const size_t need = ksplit > 1 ? (size_t)tiles * ksplit * 8192 : 0;   // LAT_PART doubles per split tile
  if (need > m->gpart_n) {
    m->gpart_n = 0;
    if ((rc = dev_alloc(m->gpart, s, sizeof(double) * need))) return rc;
    m->gpart_n = need;
  }
  return MFGP_OK;
}
// The column store of V for the model's grid and row capacity (vc_ld follows V's: a capacity
// growth reallocates it and moves the valid rows to the new stride, as ensure_v moves V's, so
// the step stays one that uploads nothing). It doubles V's memory, so it is bounded:
// VCOL_MAX per model (the headline's 8 x 270 MB fit; configs[4]'s 2.1 GB per model do not, and
// run as without a store) and a quarter of the free memory. A model that gets none runs the
// step from the compact rows. The refusal is remembered per shape: no query per step.
constexpr int64_t VCOL_MAX = int64_t(1) << 30;
int ensure_vcol(mfgp_model* m) {
  mfgp_ctx* c = m->ctx;
  const int64_t ldc = m->vld, M = m->M;
  if (m->Vc && m->vc_ld == ldc && m->vc_M == M) return MFGP_OK;
  const int64_t budget = c->vcol_budget >= 0 ? c->vcol_budget : VCOL_MAX;
  if (!m->Vc && m->vc_deny_ld == ldc && m->vc_deny_M == M && m->vc_deny_budget == budget) return MFGP_OK;
  HIP_TRY(hipStreamSynchronize(c->stream));
  // rows of the old store that stay valid at the new stride (the same grid and generation)
  const int64_t keep = m->st.vcol_keep(m->Vc && m->vc_M == M, ldc, m->vc_ld);
  Dev<void> old;   // the old store until its kept rows are copied (freed on every return)
  old.swap(m->Vc);
  const int64_t old_ld = m->vc_ld;
  m->st.vcol_reallocated();
  m->vc_ld = m->vc_M = 0;
  const size_t es = v_elem(m);
  const int64_t bytes = (int64_t)es * M * ldc;
  size_t free_b = 0, total_b = 0;
  bool ok = c->lat_vcol != 0 && ldc > 0 && M > 0 && m->V && bytes <= budget;
  if (ok && hipMemGetInfo(&free_b, &total_b) == hipSuccess) ok = (size_t)bytes <= free_b / 4;
  if (ok && dev_alloc(m->Vc, c->stream, (size_t)bytes, A_NO_DRAIN) != MFGP_OK) ok = false;   // (refused: no store)
  if (ok && old && keep > 0) {
    // (a failed copy: the new store with no valid rows, vc_ld == 0, so the next call starts over)
    HIP_TRY(hipMemcpy2DAsync(m->Vc, es * ldc, old, es * old_ld, es * keep, M, hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    m->st.vcol_rows_kept(keep);
  }
  old.reset();
  if (!ok) {
    m->vc_deny_ld = ldc;
    m->vc_deny_M = M;
    m->vc_deny_budget = budget;
    return MFGP_OK;
  }
  m->vc_ld = ldc;
  m->vc_M = M;
  return MFGP_OK;
}
// rows of the store that equal V's now
int64_t vcol_rows(const mfgp_model* m) {
  return (m->Vc && m->vc_ld == m->vld && m->vc_M == m->M) ? m->st.vcol_rows() : 0;
}
int status_error(int st) {
  if (st == INT_MIN)   // wait_flag gave up (mfgp_kernels.hip): a hand-off inside k_inc_stream never arrived
    return set_err(MFGP_ERR_DEVICE, "device synchronisation timeout in the fused append+predict launch");
  return set_err(MFGP_ERR_NOT_PD, "Matrix is not positive definite (leading minor of order %d)", st);
}

int read_status(mfgp_model* m) {
  mfgp_ctx* c = m->ctx;
  int rc = ensure_h_status(c, 1);
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(c->h_status, m->status, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  const int st = c->h_status[0];
  if (st != INT_MAX) return status_error(st);
  return MFGP_OK;
}

// The model's mapped pinned result buffer [2][M] (spec_out): host-bound predict
// outputs are written there by the kernels over the bus and kept, so that the
// predicts of an unchanged model return them (the same bits, no launch).
// Result buffers handed over by mfgp_predict_view come back here (process-wide:
// a view may outlive its model and context); ensure_spec_out takes one of at least
// the size it needs before it allocates. Bounded: beyond VIEW_POOL_MAX the
// returned buffer is freed.
struct ViewBuf {
  double* host;  // released by its owner (a model's spec_out); adopted again by owner() below
  int64_t cap;   // doubles per half ([2][cap]), then the trailer (max var, argmax) at [2 cap]
  int has_max;   // the trailer holds the fused max / argmax of the var half
  static size_t bytes(int64_t cap) { return sizeof(double) * (2 * (size_t)cap + 2); }
  Pin<double> owner() const { return Pin<double>(host, bytes(cap)); }
};
static std::mutex g_view_mu;
static std::vector<ViewBuf> g_view_pool;
constexpr size_t VIEW_POOL_MAX = 8;

int ensure_spec_out(mfgp_model* m) {
  if (m->spec_out && m->spec_cap >= m->M) return MFGP_OK;
  mfgp_ctx* c = m->ctx;
  HIP_TRY(hipStreamSynchronize(c->stream));
  m->spec_out.reset();
  m->spec_out_dev = nullptr;
  m->spec_cap = 0;
  m->spec_valid = false;
  m->spec_max = false;
  int64_t cap = m->M;
  {
    // best fit: the smallest pooled buffer that holds M (a small model does not take
    // the large buffer another model just returned)
    std::lock_guard<std::mutex> g(g_view_mu);
    size_t best = g_view_pool.size();
    for (size_t i = 0; i < g_view_pool.size(); ++i)
      if (g_view_pool[i].cap >= m->M && (best == g_view_pool.size() || g_view_pool[i].cap < g_view_pool[best].cap))
        best = i;
    if (best < g_view_pool.size()) {
      // (the pool's buffers are laid out [2][cap]: mu at 0, var at cap)
      m->spec_out = g_view_pool[best].owner();
      cap = g_view_pool[best].cap;
      g_view_pool.erase(g_view_pool.begin() + (long)best);
    }
  }
  int rc;
  // portable: a pooled buffer may serve a model of a context on another device
  if (!m->spec_out && (rc = pin_alloc(m->spec_out, ViewBuf::bytes(cap), hipHostMallocMapped | hipHostMallocPortable)))
    return rc;
  if ((rc = pin_device(m->spec_out, m->spec_out_dev))) {
    m->spec_out.reset();
    return rc;
  }
  m->spec_cap = cap;   // (with the buffer and its device address there)
  return MFGP_OK;
}

// Where the predict kernels write mu / var: the caller's buffers when both are
// device memory, else the model's result buffer (model_out_done copies it out).
static int model_out(mfgp_model* m, double* mu, double* var, double*& kmu, double*& kvar, bool& host) {
  host = !(is_device_ptr(mu) && is_device_ptr(var));
  if (!host) {
    kmu = mu;
    kvar = var;
    return MFGP_OK;
  }
  int rc = ensure_spec_out(m);
  if (rc) return rc;
  m->spec_max = false;   // (this predict computes no fused max into the trailer)
  kmu = m->spec_out_dev;
  kvar = m->spec_out_dev + m->spec_cap;
  return MFGP_OK;
}

static void model_out_done(mfgp_model* m, double* mu, double* var, bool host) {
  if (!host) return;
  if (mu != m->spec_out) std::memcpy(mu, m->spec_out, sizeof(double) * m->M);
  if (var != m->spec_out + m->spec_cap) std::memcpy(var, m->spec_out + m->spec_cap, sizeof(double) * m->M);
  m->spec_valid = true;
}

static_assert(sizeof(mfgp_model::hyp) == sizeof(mfgp_state::ModelState::factor_hyp), "the state compares all of hyp");

bool factor_current(const mfgp_model* m) { return m->st.factor_current(m->NL + m->NH, m->hyp, m->jitter); }

// Rows [factor_N, N) can be appended to the current factor (k_inc_factor).
bool can_inc_factor(const mfgp_model* m) {
  return m->st.can_inc_factor(m->NL + m->NH, m->hyp, m->jitter, m->ctx->incremental, KINC);
}

// Predict by one pass over the resident V (k_vstream): V valid for rows < v_n,
// at most KINC factor rows beyond it (the factor must be current).
bool can_vstream(const mfgp_model* m) {
  return m->ctx->incremental && m->M > 0 && m->V && m->vtiles >= ntiles_grid(m->M) &&
         m->st.can_vstream(m->NL + m->NH, KINC);
}

bool is_device_ptr(const void* p) {
  if (!p) return false;
  hipPointerAttribute_t a;
  if (hipPointerGetAttributes(&a, p) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  return a.type == hipMemoryTypeDevice;
}

int copy_rows(mfgp_model* m, int64_t at, const double* X, const double* y, int64_t k) {
  if (k <= 0) return MFGP_OK;
  if (!X || !y) return set_err(MFGP_ERR_ARG, "null data pointer with k=%lld", (long long)k);
  HIP_TRY(hipMemcpyAsync(m->X + 2 * at, X, sizeof(double) * 2 * k, hipMemcpyDefault, m->ctx->stream));
  HIP_TRY(hipMemcpyAsync(m->y + at, y, sizeof(double) * k, hipMemcpyDefault, m->ctx->stream));
  return MFGP_OK;
}
}  // namespace mfgp_host

// (the debug reads' buffers: weak symbols of the library's dynamic table since those
// entry points came, kept there)
template std::vector<char>::vector(size_t, const std::allocator<char>&);
template std::vector<float>::vector(size_t, const std::allocator<float>&);

extern "C" {

const char* mfgp_last_error(void) { return g_err.c_str(); }

#ifdef MFGP_STAMPS
// diagnostic builds only (tools/): device buffer for the kernels' phase stamps
int mfgp_debug_set_stamps(void* p) {
  HIP_TRY(set_stamps((long long*)p));
  return MFGP_OK;
}
#endif
const char* mfgp_version(void) { return "mfgp_hip 0.3 gfx950 f64 f32v"; }

int mfgp_ctx_create(int device, mfgp_ctx** out) {
  const DeviceGuard dg_(device);
  if (!out) return set_err(MFGP_ERR_ARG, "null out");
  *out = nullptr;
  int n = 0;
  HIP_TRY(hipGetDeviceCount(&n));
  if (device < 0 || device >= n) return set_err(MFGP_ERR_ARG, "device %d out of range (%d devices)", device, n);
  mfgp_ctx* c = new mfgp_ctx();
  c->device = device;
  HIP_TRY(hipStreamCreateWithFlags(&c->own, hipStreamNonBlocking));
  {
    int ncu = 0;
    if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && ncu > 0)
      c->ncu = ncu;
  }
  c->stream = c->own;
  if (const char* e = std::getenv("MFGP_DESC_ARG")) c->desc_arg = std::atoi(e) != 0;
  if (const char* e = std::getenv("MFGP_SPIN_US")) c->spin_us = std::max(0, std::atoi(e));
  if (const char* e = std::getenv("MFGP_EARLY_PD")) c->early_pd = std::atoi(e) != 0;
  if (const char* e = std::getenv("MFGP_LAT_ZCSR")) c->lat_zcsr = std::atoi(e) != 0 ? 1 : 0;
  if (const char* e = std::getenv("MFGP_RSPLIT")) {
    const int r = std::atoi(e);
    c->rsplit_force = (r == 1 || r == 2 || r == 4) ? r : 0;
  }
  if (const char* e = std::getenv("MFGP_LAT_KSPLIT")) c->lat_ksplit = std::max(0, std::min(8, std::atoi(e)));
  if (const char* e = std::getenv("MFGP_LAT_WU")) c->lat_wu = std::max(0, std::atoi(e));
  if (const char* e = std::getenv("MFGP_LAT_SELFG")) c->lat_selfg = std::atoi(e) != 0;
  if (const char* e = std::getenv("MFGP_LAT_VCOL")) {
    const int v = std::atoi(e);
    c->lat_vcol = (e[0] == 'a' || v < 0) ? -1 : (v != 0 ? 1 : 0);
  }
  if (const char* e = std::getenv("MFGP_LAT_GEMM2")) c->lat_gemm2 = std::atoi(e) != 0 ? 1 : 0;
  if (const char* e = std::getenv("MFGP_PLAN_SEP")) c->plan_sep = std::atoi(e) != 0 ? 1 : 0;
  if (const char* e = std::getenv("MFGP_TRINV_COLUMNS")) c->trinv_columns = std::atoi(e) != 0;
  if (const char* e = std::getenv("MFGP_FACTOR_DEPTH")) c->factor_depth = std::max(1, std::min(16, std::atoi(e)));
  // A/B runs: MFGP_LATTICE = 0 (V stream only), 1 (default), 2 (lattice without the size gate)
  if (const char* e = std::getenv("MFGP_LATTICE")) {
    const int v = std::atoi(e);
    c->lattice = v != 0;
    c->lat_force = v == 2;
  }
  int rc;
  if ((rc = pin_alloc(c->h_ring, sizeof(GPDesc) * RING * MAXB, hipHostMallocDefault))) return rc;
  if ((rc = dev_alloc(c->d_ring, c->stream, sizeof(GPDesc) * RING * MAXB, A_NO_DRAIN))) return rc;
  for (int i = 0; i < RING; ++i) {
    HIP_TRY(hipEventCreateWithFlags(&c->ring_ev[i], hipEventDisableTiming));
    c->ring_used[i] = false;
  }
  *out = c;
  return MFGP_OK;
}

void mfgp_ctx_destroy(mfgp_ctx* c) {
  const DeviceGuard dg_(c ? c->device : -1);
  (void)settle(c);
  if (!c) return;
  (void)hipStreamSynchronize(c->stream);
  (void)drain_timing(c);
  for (auto e : c->pool) (void)hipEventDestroy(e);
  for (int i = 0; i < RING; ++i) (void)hipEventDestroy(c->ring_ev[i]);
  if (c->own) (void)hipStreamDestroy(c->own);
  delete c;   // (its buffers free themselves)
}

int mfgp_ctx_trim(mfgp_ctx* c) {
  const DeviceGuard dg_(c ? c->device : -1);
  if (const int rc_ = settle(c)) return rc_;
  if (!c) return set_err(MFGP_ERR_ARG, "null ctx");
  HIP_TRY(hipStreamSynchronize(c->stream));
  c->vscr.reset();
  c->ws.reset();
  c->nb_dev.reset();
  c->nb_host.reset();
  return MFGP_OK;
}

// A switch of the context changes between launches: the context checked, a running
// early-return launch settled first, the stream drained.
static int ctx_idle(mfgp_ctx* c) {
  if (!c) return set_err(MFGP_ERR_ARG, "null ctx");
  if (const int rc_ = settle(c)) return rc_;
  HIP_TRY(hipStreamSynchronize(c->stream));
  return MFGP_OK;
}

int mfgp_ctx_set_nlml_chunk(mfgp_ctx* c, int max_members) {
  if (!c) return set_err(MFGP_ERR_ARG, "null ctx");
  if (max_members < 0) return set_err(MFGP_ERR_ARG, "max_members must be >= 0 (0: automatic)");
  c->nlml_chunk = std::min(max_members, MAXB);
  return MFGP_OK;
}

int mfgp_ctx_set_stream(mfgp_ctx* c, void* s) {
  if (const int rc_ = ctx_idle(c)) return rc_;
  c->stream = s ? (hipStream_t)s : c->own;
  return MFGP_OK;
}

void* mfgp_ctx_get_stream(mfgp_ctx* c) { return c ? (void*)c->stream : nullptr; }

int mfgp_ctx_synchronize(mfgp_ctx* c) {
  const DeviceGuard dg_(c ? c->device : -1);
  if (!c) return set_err(MFGP_ERR_ARG, "null ctx");
  c->early_running = false;
  int rc = ensure_h_status(c, c->async_status.size());
  if (rc) return rc;
  // the status words come back through pinned memory with the stream's last copies
  // (or straight from the mapped word the launch itself published them into)
  bool all_mapped = !c->async_status.empty();
  for (size_t i = 0; i < c->async_status.size(); ++i)
    if (!c->async_status[i].host) {
      all_mapped = false;
      HIP_TRY(hipMemcpyAsync(c->h_status + i, c->async_status[i].dev, sizeof(int), hipMemcpyDeviceToHost,
                             c->stream));
    }
  if (all_mapped && c->spin_us > 0) {
    // launches that publish their status into mapped host memory as their last act
    // (the one-GP fused step: the drop-in simulator's updt_hifi): poll those words
    // first, so that the stream synchronisation below starts when the kernel is
    // about to end and returns within its active-wait phase instead of sleeping
    // through the kernel and waking late (the outputs are visible only after it)
    const auto t0 = std::chrono::steady_clock::now();
    for (size_t i = 0; i < c->async_status.size(); ++i) {
      const volatile int* w = reinterpret_cast<const volatile int*>(c->async_status[i].host);
      while (*w == STATUS_UNSET) {
        __builtin_ia32_pause();
        if (std::chrono::steady_clock::now() - t0 > std::chrono::microseconds(c->spin_us)) break;
      }
    }
  }
  HIP_TRY(hipStreamSynchronize(c->stream));
  for (size_t i = 0; i < c->async_status.size(); ++i) {
    const auto& as = c->async_status[i];
    if (as.host) {
      c->h_status[i] = *reinterpret_cast<volatile int*>(as.host);
      if (c->h_status[i] == STATUS_UNSET)   // not published (cannot happen with cell tiles): read the word
        HIP_TRY(hipMemcpy(c->h_status + i, as.dev, sizeof(int), hipMemcpyDeviceToHost));
    }
  }
  for (size_t i = 0; i < c->async_status.size(); ++i) {
    const int st = c->h_status[i];
    if (st == INT_MAX) continue;
    // a failed factor leaves its model without one: the next use refactors (and
    // raises again), instead of serving the failed factor and its V
    mfgp_model* m = c->async_status[i].m;
    m->st.factor_lost(FactorLost::AsyncFailed);
    m->st.v_dropped();
    m->spec_valid = false;
    if (rc == MFGP_OK) rc = status_error(st);
  }
  c->async_status.clear();
  return rc;
}

int mfgp_ctx_set_incremental(mfgp_ctx* c, int enable) {
  if (const int rc_ = ctx_idle(c)) return rc_;
  c->incremental = enable != 0;
  return MFGP_OK;
}

int mfgp_ctx_set_fused(mfgp_ctx* c, int enable) {
  if (const int rc_ = ctx_idle(c)) return rc_;
  c->fused = enable != 0;
  return MFGP_OK;
}

int mfgp_ctx_set_deferred_appends(mfgp_ctx* c, int enable) {
  if (const int rc_ = ctx_idle(c)) return rc_;
  c->deferred = enable != 0;
  return MFGP_OK;
}

int mfgp_ctx_set_lattice(mfgp_ctx* c, int enable) {
  if (const int rc_ = ctx_idle(c)) return rc_;
  c->lattice = enable != 0;
  c->lat_force = enable == 2;
  return MFGP_OK;
}

int mfgp_ctx_set_lattice_vcol(mfgp_ctx* c, int mode) {
  if (const int rc_ = ctx_idle(c)) return rc_;
  c->lat_vcol = mode < 0 ? -1 : (mode != 0 ? 1 : 0);
  return MFGP_OK;
}

int mfgp_ctx_set_vcol_budget(mfgp_ctx* c, int64_t bytes) {
  if (const int rc_ = ctx_idle(c)) return rc_;
  c->vcol_budget = bytes < 0 ? -1 : bytes;
  return MFGP_OK;
}

int mfgp_ctx_set_concurrent(mfgp_ctx* c, int enable) {
  if (const int rc_ = ctx_idle(c)) return rc_;
  c->concurrent = enable != 0;
  return MFGP_OK;
}

int mfgp_ctx_enable_timing(mfgp_ctx* c, int enable) {
  if (!c) return set_err(MFGP_ERR_ARG, "null ctx");
  if (const int rc_ = settle(c)) return rc_;   // (a running early-return launch first)
  c->timing = (enable == 2) ? 2 : (enable != 0 ? 1 : 0);
  return MFGP_OK;
}

int mfgp_ctx_set_timing_stride(mfgp_ctx* c, int64_t stride) {
  if (!c) return set_err(MFGP_ERR_ARG, "null ctx");
  if (const int rc_ = settle(c)) return rc_;   // (a running early-return launch first)
  if (stride < 1) return set_err(MFGP_ERR_ARG, "timing stride must be >= 1");
  c->timing_stride = stride;
  c->timing_seq = 0;
  return MFGP_OK;
}

int mfgp_ctx_get_timing(mfgp_ctx* c, double* pm, int64_t* pn, double* fm, int64_t* fn) {
  if (!c) return set_err(MFGP_ERR_ARG, "null ctx");
  if (const int rc_ = settle(c)) return rc_;   // (a running early-return launch first)
  int rc = drain_timing(c);
  if (rc) return rc;
  if (pm) *pm = c->t_predict;
  if (pn) *pn = c->n_predict;
  if (fm) *fm = c->t_factor;
  if (fn) *fn = c->n_factor;
  return MFGP_OK;
}

int mfgp_ctx_reset_timing(mfgp_ctx* c) {
  if (!c) return set_err(MFGP_ERR_ARG, "null ctx");
  if (const int rc_ = settle(c)) return rc_;   // (a running early-return launch first)
  int rc = drain_timing(c);
  c->t_predict = c->t_factor = 0.0;
  c->n_predict = c->n_factor = 0;
  return rc;
}

int mfgp_model_create(mfgp_ctx* c, int kind, int dtype, const double* hyp, int nhyp, double jitter,
                      mfgp_model** out) {
  const DeviceGuard dg_(c ? c->device : -1);
  if (const int rc_ = settle(c)) return rc_;
  if (!c || !out) return set_err(MFGP_ERR_ARG, "null ctx/out");
  *out = nullptr;
  if (kind != MFGP_SF && kind != MFGP_MF) return set_err(MFGP_ERR_ARG, "kind must be MFGP_SF or MFGP_MF");
  if (dtype != MFGP_F64 && dtype != MFGP_F32) return set_err(MFGP_ERR_ARG, "dtype must be MFGP_F64 or MFGP_F32");
  const int want = kind == MFGP_SF ? 4 : 9;
  if (!hyp || nhyp != want)
    return set_err(MFGP_ERR_ARG, "Hyperparameters must be of length 4 (single-fidelity) or 9 (multi-fidelity)");
  ModelGuard guard(new mfgp_model());   // until *out is set, every failing return destroys it
  mfgp_model* m = guard.get();
  m->ctx = c;
  m->kind = kind;
  m->dtype = dtype;
  m->nhyp = nhyp;
  std::memcpy(m->hyp, hyp, sizeof(double) * nhyp);
  m->jitter = jitter;
  bump_serial(m);
  int rc;
  if ((rc = dev_alloc(m->status, c->stream, sizeof(int), A_NO_DRAIN))) return rc;
  {
    // "no failure" until a step writes it: a step whose kernels all skip (a gated
    // model of mfgp_batch_sample_points) must not read an uninitialised word
    const int ok = INT_MAX;
    HIP_TRY(hipMemcpy(m->status, &ok, sizeof(int), hipMemcpyHostToDevice));
  }
  if ((rc = ensure_cap(m, 63))) return rc;
  *out = guard.release();
  return MFGP_OK;
}

void mfgp_model_destroy(mfgp_model* m) {
  const DeviceGuard dg_(m ? m->ctx->device : -1);
  (void)settle(m ? m->ctx : nullptr);
  if (!m) return;
  if (m->ctx) {
    (void)hipStreamSynchronize(m->ctx->stream);
    // an ASYNC batch's status word of this model dies with it (the work is done)
    auto& as = m->ctx->async_status;
    as.erase(std::remove_if(as.begin(), as.end(), [m](const mfgp_ctx::AsyncStatus& e) { return e.m == m; }),
             as.end());
  }
  delete m;   // (its buffers and records free themselves)
}

int mfgp_ctx_planner_stats(mfgp_ctx* c, int64_t* out, int n, int reset) {
  if (!c || (n > 0 && !out)) return set_err(MFGP_ERR_ARG, "null ctx/out");
  if (const int rc_ = settle(c)) return rc_;   // (a running early-return launch first)
  for (int i = 0; i < n && i < PLAN_NSTATS; ++i) out[i] = c->plan_stats[i];
  if (reset)
    for (int64_t& v : c->plan_stats) v = 0;
  return MFGP_OK;
}

int mfgp_clone(const mfgp_model* src, mfgp_model** out) {
  const Entry entry(src);
  int rc = entry.rc;
  if (rc) return rc;
  if (!out) return set_err(MFGP_ERR_ARG, "null out");
  mfgp_ctx* c = src->ctx;
  mfgp_model* m = nullptr;
  if ((rc = mfgp_model_create(c, src->kind, src->dtype, src->hyp, src->nhyp, src->jitter, &m))) return rc;
  ModelGuard guard(m);   // until *out is set, every failing return destroys the copy
  if ((rc = ensure_cap(m, src->cap))) return rc;
  // same capacity => same ld: the factor copies verbatim
  const int64_t n = src->NL + src->NH;
  m->NL = src->NL;
  m->NH = src->NH;
  if (n > 0) {
    HIP_TRY(hipMemcpyAsync(m->X, src->X, sizeof(double) * 2 * n, hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(m->y, src->y, sizeof(double) * n, hipMemcpyDeviceToDevice, c->stream));
  }
  if (src->st.factored && src->ld == m->ld) {
    HIP_TRY(hipMemcpyAsync(m->A, src->A, sizeof(double) * src->ld * src->ld, hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(m->Linv, src->Linv, sizeof(double) * (src->ld / NB) * TILE, hipMemcpyDeviceToDevice,
                           c->stream));
    HIP_TRY(hipMemcpyAsync(m->zv, src->zv, sizeof(double) * src->cap, hipMemcpyDeviceToDevice, c->stream));
    m->st.adopt_factor(src->st);
  }
  if (src->M > 0) {
    if ((rc = dev_alloc(m->grid, c->stream, sizeof(double) * 2 * src->M, A_NO_DRAIN))) return rc;
    HIP_TRY(hipMemcpyAsync(m->grid, src->grid, sizeof(double) * 2 * src->M, hipMemcpyDeviceToDevice, c->stream));
    m->M = m->Mcap = src->M;
    m->lat = src->lat;
    m->hax = src->hax;
    m->hay = src->hay;
    // resident V (a deepcopy'd model keeps appending to the copy, sim:339)
    if (m->st.factored && src->V && src->st.v_n > 0 && src->vld == round_up(m->cap, PRB)) {
      if ((rc = ensure_v(m))) return rc;
      HIP_TRY(hipMemcpyAsync(m->V, src->V, v_elem(src) * (size_t)src->vtiles * src->vld * PBM,
                             hipMemcpyDeviceToDevice, c->stream));
      m->st.adopt_v(src->st);
    }
  }
  HIP_TRY(hipStreamSynchronize(c->stream));
  *out = guard.release();
  return MFGP_OK;
}

int mfgp_model_set_hyp(mfgp_model* m, const double* hyp, int nhyp, double jitter) {
  const Entry entry(m);
  int rc = entry.rc;
  if (rc) return rc;
  if (!hyp || nhyp != m->nhyp)
    return set_err(MFGP_ERR_ARG, "Hyperparameters must be of length 4 (single-fidelity) or 9 (multi-fidelity)");
  if (jitter != m->jitter || std::memcmp(hyp, m->hyp, sizeof(double) * nhyp) != 0) {
    m->spec_valid = false;
    m->st.new_generation();   // (V's rows stay counted: the factor's hyp test refactors before V is read)
    bump_serial(m);
  }
  std::memcpy(m->hyp, hyp, sizeof(double) * nhyp);
  m->jitter = jitter;
  return MFGP_OK;
}

// Is the grid a lattice of two strictly monotone axes, one coordinate constant
// along runs of consecutive cells (meshgrid order, either way round)?
GridLattice detect_lattice(const double* g, int64_t M) {
  GridLattice L{};
  if (M < 1 || M > INT_MAX) return L;
  auto monotone = [](const double* v, int64_t n, int64_t stride) {
    if (n < 2) return v[0] == v[0];
    const bool up = v[stride] > v[0];
    for (int64_t i = 1; i < n; ++i) {
      const double a = v[(i - 1) * stride], b = v[i * stride];
      if (!(up ? b > a : b < a)) return false;
    }
    return true;
  };
  for (int s = 0; s < 2; ++s) {       // s = the coordinate constant along a run
    const int f = 1 - s;
    int64_t run = 1;
    while (run < M && g[2 * run + s] == g[s]) ++run;
    if (M % run) continue;
    bool ok = true;
    for (int64_t i = 0; i < M && ok; ++i)
      ok = g[2 * i + s] == g[2 * (i - i % run) + s] && g[2 * i + f] == g[2 * (i % run) + f];
    const int64_t ns = M / run;
    if (!ok || !monotone(g + s, ns, 2 * run) || !monotone(g + f, run, 2)) continue;
    // slow axis: values g[2 j run + s], stride run; fast axis: g[2 j + f], stride 1
    const int64_t xn = s == 0 ? ns : run, xst = s == 0 ? run : 1;
    const int64_t yn = s == 0 ? run : ns, yst = s == 0 ? 1 : run;
    const double x0 = g[0], x1 = g[2 * (xn - 1) * xst];
    const double y0 = g[1], y1 = g[2 * (yn - 1) * yst + 1];
    L.nx = (int)xn;
    L.ny = (int)yn;
    L.sx = xst;
    L.sy = yst;
    L.x0 = x0;
    L.y0 = y0;
    L.xinv = xn > 1 ? (double)(xn - 1) / (x1 - x0) : 0.0;
    L.yinv = yn > 1 ? (double)(yn - 1) / (y1 - y0) : 0.0;
    return L;
  }
  return L;
}

int mfgp_set_grid(mfgp_model* m, const double* xs, int64_t M) {
  const Entry entry(m);
  int rc = entry.rc;
  if (rc) return rc;
  if (M < 0 || (M > 0 && !xs)) return set_err(MFGP_ERR_ARG, "bad grid");
  mfgp_ctx* c = m->ctx;
  // The new grid goes to the device first: into a buffer of its own where the model's is
  // too small, so that a refused allocation or a failed copy leaves the model on its old
  // grid, untouched. Where it fits, the copy overwrites the old grid in place: that one is
  // gone first, and a failed copy leaves a model without a grid (M == 0).
  Dev<double> grown;
  if (M > m->Mcap && (rc = dev_alloc(grown, c->stream, sizeof(double) * 2 * M))) return rc;
  auto old_grid_gone = [m] {
    m->M = 0;
    m->st.v_dropped();   // V columns belong to the previous grid
    m->spec_valid = false;
    m->st.new_generation();
    bump_serial(m);
    m->lat = GridLattice{};
    m->hax.clear();
    m->hay.clear();
  };
  if (!grown) old_grid_gone();
  double* const g = grown ? grown.get() : m->grid.get();
  std::vector<double> h(2 * (size_t)M);
  if (M > 0) {
    HIP_TRY(hipMemcpyAsync(g, xs, sizeof(double) * 2 * M, hipMemcpyDefault, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpy(h.data(), g, sizeof(double) * 2 * M, hipMemcpyDeviceToHost));
  } else {
    HIP_TRY(hipStreamSynchronize(c->stream));
  }
  if (grown) {
    old_grid_gone();
    m->grid.swap(grown);
    m->Mcap = M;
  }
  m->M = M;
  if (M > 0) {
    m->lat = detect_lattice(h.data(), M);
    m->hax.assign((size_t)std::max(m->lat.nx, 0), 0.0);
    m->hay.assign((size_t)std::max(m->lat.ny, 0), 0.0);
    for (int i = 0; i < m->lat.nx; ++i) m->hax[i] = h[2 * (i * m->lat.sx)];
    for (int i = 0; i < m->lat.ny; ++i) m->hay[i] = h[2 * (i * m->lat.sy) + 1];
  }
  return MFGP_OK;
}

int mfgp_set_data(mfgp_model* m, const double* XL, const double* yL, int64_t NL, const double* XH,
                  const double* yH, int64_t NH) {
  const Entry entry(m);
  int rc = entry.rc;
  if (rc) return rc;
  if (NL < 0 || NH < 0) return set_err(MFGP_ERR_ARG, "negative sizes");
  if (m->kind == MFGP_SF && NL != 0) return set_err(MFGP_ERR_ARG, "SF model takes its data in the H slots");
  if ((rc = ensure_cap(m, NL + NH))) return rc;   // (refused: the model, its serial and kept result as they were)
  m->spec_valid = false;
  bump_serial(m);
  m->NL = NL;
  m->NH = NH;
  if ((rc = copy_rows(m, 0, XL, yL, NL))) return rc;
  if ((rc = copy_rows(m, NL, XH, yH, NH))) return rc;
  m->st.factor_lost(FactorLost::RowsReplaced);
  return factor_one(m);
}


int mfgp_append(mfgp_model* m, const double* X, const double* y, int64_t k) {
  const Entry entry(m);
  int rc = entry.rc;
  if (rc) return rc;
  if (k < 0) return set_err(MFGP_ERR_ARG, "negative k");
  const int64_t n = m->NL + m->NH;
  if ((rc = ensure_cap(m, n + k))) return rc;   // (refused: the model, its serial and kept result as they were)
  m->spec_valid = false;
  if (k > 0) bump_serial(m);
  const bool spec = m->pred_since_append;   // the last append was followed by a predict
  m->pred_since_append = false;
  if (k > 0 && (!X || !y)) return set_err(MFGP_ERR_ARG, "null data pointer with k=%lld", (long long)k);
  m->NH += k;
  if (!m->ctx->incremental) m->st.factor_lost(FactorLost::NotIncremental);   // reference behaviour: refactor from scratch
  const bool staged = m->ctx->deferred && can_inc_factor(m);   // the next factor user runs the append
  const bool sp = !staged && spec && m->ctx->fused && k > 0 && m->M > 0 && can_inc_factor(m) && m->V &&
                  m->st.v_at_factor() && m->vtiles >= ntiles_grid(m->M);
  m->NH -= k;
  // the speculative step carries the rows in its launch (batch_run appends them)
  if (sp) return spec_append_predict(m, X, y, k);
  if ((rc = copy_rows(m, n, X, y, k))) return rc;
  m->NH += k;
  if (staged) return MFGP_OK;
  return update_factor(m);
}

int mfgp_truncate(mfgp_model* m, int64_t n_keep_hifi) {
  const Entry entry(m);
  int rc = entry.rc;
  if (rc) return rc;
  if (n_keep_hifi != m->NH) m->spec_valid = false;
  if (n_keep_hifi < 0 || n_keep_hifi > m->NH) return set_err(MFGP_ERR_ARG, "bad truncate size");
  if (n_keep_hifi != m->NH) {
    m->NH = n_keep_hifi;
    bump_serial(m);
    m->st.rows_cut(m->NL + m->NH);
  }
  return MFGP_OK;
}

static int predict_view(mfgp_model* m, double** mu, double** var, void** view, int* running) {
  const DeviceGuard dg_(m ? m->ctx->device : -1);
  int rc = check_model(m);
  if (rc) return rc;
  if (!mu || !var || !view) return set_err(MFGP_ERR_ARG, "null output");
  *mu = *var = nullptr;
  *view = nullptr;
  if (running) *running = 0;
  if (running && m->ctx->early_running && m->spec_valid && m->spec_out && m->M > 0 && factor_current(m)) {
    // the result of the eager append still being computed into the buffer handed
    // over here: the caller wraps it, then settles (mfgp_ctx_synchronize) before it
    // reads it or lets anyone else
    *running = 1;
    m->pred_since_append = true;
  } else {
    if ((rc = settle(m->ctx))) return rc;
    if (m->M == 0) return mfgp_predict(m, nullptr, nullptr);
    if ((rc = ensure_spec_out(m))) return rc;
    // the predict's host outputs are the result buffer itself: no copy
    if ((rc = mfgp_predict(m, m->spec_out, m->spec_out + m->spec_cap))) return rc;
  }
  // the buffer is the caller's now: the model's next host-bound predict takes another
  ViewBuf* v = new ViewBuf{m->spec_out.release(), m->spec_cap, m->spec_max ? 1 : 0};
  *mu = v->host;
  *var = v->host + v->cap;
  *view = v;
  m->spec_out_dev = nullptr;
  m->spec_cap = 0;
  m->spec_valid = false;
  m->spec_max = false;
  return MFGP_OK;
}

int mfgp_view_max(const void* view, double* vmax, int64_t* argmax, int* valid) {
  if (!view || !vmax || !argmax || !valid) return set_err(MFGP_ERR_ARG, "null view/output");
  const ViewBuf* v = static_cast<const ViewBuf*>(view);
  *valid = v->has_max;
  if (v->has_max) {
    *vmax = v->host[2 * v->cap];
    std::memcpy(argmax, v->host + 2 * v->cap + 1, sizeof(int64_t));
  }
  return MFGP_OK;
}

int mfgp_predict_view(mfgp_model* m, double** mu, double** var, void** view) {
  return predict_view(m, mu, var, view, nullptr);
}

int mfgp_predict_view_running(mfgp_model* m, double** mu, double** var, void** view, int* running) {
  if (!running) return set_err(MFGP_ERR_ARG, "null output");
  return predict_view(m, mu, var, view, running);
}

int mfgp_release_view(void* view) {
  if (!view) return MFGP_OK;
  ViewBuf* v = static_cast<ViewBuf*>(view);
  bool keep = false;
  {
    std::lock_guard<std::mutex> g(g_view_mu);
    if (g_view_pool.size() < VIEW_POOL_MAX) {
      g_view_pool.push_back(*v);
      keep = true;
    }
  }
  if (!keep) v->owner().reset();
  delete v;
  return MFGP_OK;
}

int mfgp_predict(mfgp_model* m, double* mu, double* var) {
  const Entry entry(m);
  int rc = entry.rc;
  if (rc) return rc;
  mfgp_ctx* c = m->ctx;
  if (m->M > 0 && (!mu || !var)) return set_err(MFGP_ERR_ARG, "null output");
  m->pred_since_append = true;
  if (m->spec_valid && factor_current(m)) {   // kept from the last predict or the append (spec_append_predict)
    const size_t b = sizeof(double) * (size_t)m->M;
    if (is_device_ptr(mu) && is_device_ptr(var)) {
      HIP_TRY(hipMemcpyAsync(mu, m->spec_out_dev, b, hipMemcpyDeviceToDevice, c->stream));
      HIP_TRY(hipMemcpyAsync(var, m->spec_out_dev + m->spec_cap, b, hipMemcpyDeviceToDevice, c->stream));
      HIP_TRY(hipStreamSynchronize(c->stream));
    } else {
      if (mu != m->spec_out) std::memcpy(mu, m->spec_out, b);
      if (var != m->spec_out + m->spec_cap) std::memcpy(var, m->spec_out + m->spec_cap, b);
    }
    return MFGP_OK;
  }
  if (m->M > 0 && !factor_current(m) && can_inc_factor(m)) {
    // a staged (deferred) append: the bordered append and the one-pass predict
    // as one launch when V is resident (the batched path for one model)
    double *kmu = nullptr, *kvar = nullptr;
    bool host = false;
    if ((rc = model_out(m, mu, var, kmu, kvar, host))) return rc;
    rc = batch_run(&m, 1, nullptr, nullptr, nullptr, kmu, kvar, nullptr, nullptr, MFGP_ASYNC, true, true);
    if (rc == MFGP_OK) rc = mfgp_ctx_synchronize(c);
    if (rc == MFGP_OK) model_out_done(m, mu, var, host);
    if (rc != MFGP_OK) m->st.factor_lost(FactorLost::StepFailed);   // a failed step leaves no usable factor
    return rc;
  }
  if ((rc = update_factor(m))) return rc;
  if (m->M == 0) return MFGP_OK;
  if ((rc = ensure_v(m))) return rc;
  double *kmu = nullptr, *kvar = nullptr;
  bool host = false;
  if ((rc = model_out(m, mu, var, kmu, kvar, host))) return rc;
  int slot;
  GPDesc* hd = acquire_slot(c, slot, rc);
  if (!hd) return rc;
  fill_desc(hd[0], m);
  hd[0].mu = kmu;
  hd[0].var = kvar;
  const int rb = set_res_out(m, hd[0], -1);
  const bool vst = can_vstream(m);
  set_vstream_rows(hd[0], m);
  set_rsplit(c, hd, 1);
  if (!vst && (rc = assign_predict_scratch(c, hd, 1))) return rc;
  const GPDesc* dd = nullptr;
  if ((rc = upload_slot(c, slot, 1, &dd))) return rc;
  if ((rc = vst ? enqueue_vstream(c, dd, hd, 1) : enqueue_predict(c, dd, hd, 1))) return rc;
  (vst ? m->cnt[N_VSTREAM] : m->cnt[N_FULL_PREDICT]) += 1;
  m->st.predict_enqueued(vst ? Predict::VStream : Predict::Full, m->NL + m->NH, rb);
  if ((rc = release_slot(c, slot))) return rc;
  HIP_TRY(hipStreamSynchronize(c->stream));
  model_out_done(m, mu, var, host);
  return MFGP_OK;
}

int mfgp_model_serial(const mfgp_model* m, uint64_t* serial) {
  if (!m || !serial) return set_err(MFGP_ERR_ARG, "null model/out");
  *serial = m->serial;
  return MFGP_OK;
}

int64_t mfgp_model_n(const mfgp_model* m) { return m ? m->NL + m->NH : -1; }

int mfgp_model_stats(const mfgp_model* m, int64_t* out, int n) {
  if (!m || !out) return set_err(MFGP_ERR_ARG, "null model/out");
  if (const int rc_ = settle(m->ctx)) return rc_;
  // off-lattice training rows the last lattice step's Z units found (lidx = -1,
  // the step's "virtual" K rows): the counts they published, read back from the
  // device (both parts; an MF hifi row off the lattice counts in each)
  int64_t virt = 0;
  if (n > 9 && m->zvl && m->cnt[N_LATTICE] > 0) {
    int nv[2] = {0, 0};
    HIP_TRY(hipStreamSynchronize(m->ctx->stream));
    HIP_TRY(hipMemcpy(&nv[0], m->zvl, sizeof(int), hipMemcpyDeviceToHost));
    if (m->kind == MFGP_MF) HIP_TRY(hipMemcpy(&nv[1], m->zvl + m->zb_rows + 1, sizeof(int), hipMemcpyDeviceToHost));
    virt = (int64_t)nv[0] + nv[1];
  }
  const int64_t v[20] = {m->st.factored ? m->st.factor_N : -1, m->st.v_n, m->cnt[N_FULL_FACTOR], m->cnt[N_INC_FACTOR],
                         m->cnt[N_FULL_PREDICT], m->cnt[N_VSTREAM], m->lat.nx, m->lat.ny, m->cnt[N_LATTICE], virt,
                         m->cnt[N_LATTICE_ARG], m->cnt[N_LATTICE_G2], m->cnt[N_POST_COPY], m->cnt[N_EARLY_PD],
                         m->cnt[N_LOOK_BORDER], m->cnt[N_LOOK_QUERY], m->cnt[N_SAMPLE_SOLVE], m->cnt[N_SAMPLE_GEMM],
                         m->cnt[N_LATTICE_VCOL], m->cnt[N_VCOL_ROWS]};
  for (int i = 0; i < n && i < 20; ++i) out[i] = v[i];
  return MFGP_OK;
}
// Tests only: the resident V's n = min(v_n, n_max) leading rows as doubles, v_out[i * M + c] =
// V(i, c), and the column store's, vc_out[c * n + i] (either may be null); *rows = n, *vc_rows
// = the store's valid rows (0: none), both or neither.
int mfgp_debug_read_v(mfgp_model* m, double* v_out, double* vc_out, int64_t n_max, int64_t* rows, int64_t* vc_rows) {
  const Entry entry(m);
  int rc = entry.rc;
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(m->ctx->stream));
  const int64_t n = m->V ? std::min(m->st.v_n, std::max<int64_t>(n_max, 0)) : 0, M = m->M;
  const int64_t vcn = vcol_rows(m);
  if (rows) *rows = n;
  if (vc_rows) *vc_rows = vcn;
  const size_t es = v_elem(m);
  auto widen = [&](const std::vector<char>& raw, size_t e) {
    return es == 8 ? reinterpret_cast<const double*>(raw.data())[e]
                   : (double)reinterpret_cast<const float*>(raw.data())[e];
  };
  if (v_out && n > 0 && M > 0) {
    std::vector<char> raw(es * (size_t)m->vtiles * m->vld * PBM);
    HIP_TRY(hipMemcpy(raw.data(), m->V, raw.size(), hipMemcpyDeviceToHost));
    for (int64_t i = 0; i < n; ++i)
      for (int64_t c = 0; c < M; ++c) v_out[i * M + c] = widen(raw, (size_t)((c / PBM) * m->vld * PBM + i * PBM + c % PBM));
  }
  if (vc_out && n > 0 && M > 0 && m->Vc) {
    std::vector<char> raw(es * (size_t)m->vc_M * m->vc_ld);
    HIP_TRY(hipMemcpy(raw.data(), m->Vc, raw.size(), hipMemcpyDeviceToHost));
    for (int64_t c = 0; c < M; ++c)
      for (int64_t i = 0; i < n; ++i) vc_out[c * n + i] = widen(raw, (size_t)(c * m->vc_ld + i));
  }
  return MFGP_OK;
}
// Tests only: the explicit inverse F = L^-1 the lattice steps keep, rows and columns [0, n), n =
// min(F's current rows, n_max), as doubles row-major f_out[i * n + j] (zeros above the diagonal);
// *rows = n (0: the model holds no current F).
int mfgp_debug_read_f(mfgp_model* m, double* f_out, int64_t n_max, int64_t* rows) {
  const Entry entry(m);
  int rc = entry.rc;
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(m->ctx->stream));
  const bool ff = m->dtype == MFGP_F32 && m->Ff;
  const int64_t n = m->F ? std::min(m->st.F.rows(m->st.gen), std::max<int64_t>(n_max, 0)) : 0;
  if (rows) *rows = n;
  if (!f_out || n == 0) return MFGP_OK;
  const int64_t ld = m->F_ld, tot = fblk_size(ld);
  std::vector<double> h((size_t)tot);
  if (ff) {
    std::vector<float> hf((size_t)tot);
    HIP_TRY(hipMemcpy(hf.data(), m->Ff, sizeof(float) * tot, hipMemcpyDeviceToHost));
    for (int64_t e = 0; e < tot; ++e) h[e] = (double)hf[e];
  } else {
    HIP_TRY(hipMemcpy(h.data(), m->F, sizeof(double) * tot, hipMemcpyDeviceToHost));
  }
  for (int64_t i = 0; i < n; ++i)
    for (int64_t j = 0; j < n; ++j)
      f_out[i * n + j] = j <= i ? h[(size_t)(fblk_off(j / 64, ld) + (i - 64 * (j / 64)) * 64 + j % 64)] : 0.0;
  return MFGP_OK;
}
// Tests only: what the library holds now, {device buffers, their bytes, pinned buffers, their
// bytes}, the view pool's buffers and the views handed out included.
int mfgp_debug_live(int64_t out[4]) {
  if (!out) return set_err(MFGP_ERR_ARG, "null out");
  out[0] = live_dev.count.load(std::memory_order_relaxed);
  out[1] = live_dev.bytes.load(std::memory_order_relaxed);
  out[2] = live_pin.count.load(std::memory_order_relaxed);
  out[3] = live_pin.bytes.load(std::memory_order_relaxed);
  return MFGP_OK;
}
int64_t mfgp_model_nl(const mfgp_model* m) { return m ? m->NL : -1; }
int64_t mfgp_model_m(const mfgp_model* m) { return m ? m->M : -1; }

int mfgp_get_factor(mfgp_model* m, double* L_out) {
  const Entry entry(m);
  int rc = entry.rc;
  if (rc) return rc;
  if ((rc = update_factor(m))) return rc;
  const int64_t N = m->NL + m->NH;
  if (N == 0) return MFGP_OK;
  std::vector<double> cm((size_t)m->ld * N);
  HIP_TRY(hipMemcpyAsync(cm.data(), m->A, sizeof(double) * m->ld * N, hipMemcpyDeviceToHost, m->ctx->stream));
  HIP_TRY(hipStreamSynchronize(m->ctx->stream));
  for (int64_t i = 0; i < N; ++i)
    for (int64_t j = 0; j < N; ++j) L_out[i * N + j] = (j <= i) ? cm[(size_t)j * m->ld + i] : 0.0;
  return MFGP_OK;
}

}  // extern "C"
