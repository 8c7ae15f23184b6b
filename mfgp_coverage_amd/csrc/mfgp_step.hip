// The step engine of libmfgp_hip.so: the descriptor ring, the enqueue_* functions (one
// set of launches per kind of work), the factor updates of one model, batch_run -- the
// shared driver of the batched entry points -- with the lattice step's planning
// (plan_lat over mfgp_lat_plan.h), and the mfgp_batch_* entry points.
#include <chrono>
#include <cmath>
#include <cstring>

#include "mfgp_host.h"
#include "mfgp_lat_plan.h"

using namespace mfgp;
using namespace mfgp_host;

static_assert(mfgp_lat_plan::WU_MAX == LAT_WU_MAX && mfgp_lat_plan::KSTAGE == ZKS, "mfgp_lat_plan.h restates these");

namespace mfgp_host __attribute__((visibility("hidden"))) {

static hipEvent_t ev_get(mfgp_ctx* c) {
  if (!c->pool.empty()) {
    hipEvent_t e = c->pool.back();
    c->pool.pop_back();
    return e;
  }
  hipEvent_t e = nullptr;
  (void)hipEventCreate(&e);
  return e;
}

static int ev_begin(mfgp_ctx* c, EvPair& p, int kind) {
  p.a = p.b = nullptr;
  if (!c->timing || (c->timing == 2 && kind != 0)) return MFGP_OK;
  if (c->timing_seq++ % c->timing_stride != 0) return MFGP_OK;
  p.a = ev_get(c);
  p.b = ev_get(c);
  p.kind = kind;
  HIP_TRY(hipEventRecord(p.a, c->stream));
  return MFGP_OK;
}

static int ev_end(mfgp_ctx* c, EvPair& p) {
  if (!p.a) return MFGP_OK;
  HIP_TRY(hipEventRecord(p.b, c->stream));
  c->pending.push_back(p);
  return MFGP_OK;
}

GPDesc* acquire_slot(mfgp_ctx* c, int& slot, int& rc) {
  slot = c->ring_pos;
  c->ring_pos = (c->ring_pos + 1) % RING;
  rc = MFGP_OK;
  if (c->ring_used[slot]) {
    hipError_t e = hipEventSynchronize(c->ring_ev[slot]);
    if (e != hipSuccess) {
      rc = set_err(MFGP_ERR_DEVICE, "hipEventSynchronize: %s", hipGetErrorString(e));
      return nullptr;
    }
  }
  return c->h_ring + (size_t)slot * MAXB;
}

int upload_slot(mfgp_ctx* c, int slot, int count, const GPDesc** dptr) {
  HIP_TRY(hipMemcpyAsync(c->d_ring + (size_t)slot * MAXB, c->h_ring + (size_t)slot * MAXB,
                         sizeof(GPDesc) * count, hipMemcpyHostToDevice, c->stream));
  *dptr = c->d_ring + (size_t)slot * MAXB;
  return MFGP_OK;
}

int release_slot(mfgp_ctx* c, int slot) {
  HIP_TRY(hipEventRecord(c->ring_ev[slot], c->stream));
  c->ring_used[slot] = true;
  return MFGP_OK;
}
// A slot whose descriptors went into a launch by value (kernel argument: copied at
// the launch call) and were never uploaded: nothing on the stream reads it, so it
// needs no event (one hipEventRecord less per step: the drop-in step's host time).
static void release_slot_unread(mfgp_ctx* c, int slot) { c->ring_used[slot] = false; }

// A model's status word to check at the next mfgp_ctx_synchronize. One entry per
// model: every entry of a model would read the same device word (its value after
// the model's last launch), so repeated ASYNC steps add no copies to the sync. A
// model's entry that the one-GP fused launch publishes into mapped memory
// (host != null) is replaced by the device word when a later step does not.
static void add_async_status(mfgp_ctx* c, mfgp_model* m) {
  for (auto& a : c->async_status)
    if (a.m == m) {
      a.host = nullptr;   // (a later launch of this model may not publish: read the word)
      return;
    }
  c->async_status.push_back({m, m->status, nullptr});
}

// ---- lattice-separable step ----
static bool lat_cond_ok(const mfgp_model* m) {
  const Hyp h = derive_hyp(m->kind, m->hyp, m->jitter);
  const double noise = (m->kind == MFGP_SF ? h.noiseL : std::min(h.noiseL, h.noiseH)) + h.jitter;
  return noise > 0.0 && h.kss / noise <= LAT_RMAX;
}
// Z units of the lattice-axis form: parts x ceil(ny / zq), zq lattice y-rows each
// (two per thread group of tabw threads)
static int lat_zq(const mfgp_model* m) { return (int)(2 * NT / lat_tabw(m)); }
static int64_t lat_nzu(const mfgp_model* m) {
  return (m->kind == MFGP_SF ? 1 : 2) * ((m->lat.ny + lat_zq(m) - 1) / lat_zq(m));
}
// Can the bordered append of rows [n0, N) and its predict take k_inc_lat?
static bool lat_eligible(const mfgp_model* m, int64_t n0) {
  const int64_t k = m->NL + m->NH - n0;
  if (!m->ctx->lattice || m->lat.nx <= 0 || m->M <= 0 || k < 1 || k > KINC || n0 < 1) return false;
  if (lat_tabw(m) > NT) return false;   // a Z unit's thread per lattice column
  if ((n0 + 63) / 64 > LAT_NWB_MAX) return false;   // a w unit's blocks
  if (!lat_cond_ok(m)) return false;
  return m->res && m->st.lat_depth_ok(n0, LAT_MAXD);
}
// The kernels' uniform test (inc_gather_fast, lat_wblock) on the host, for the path counter:
// is every new row the lattice cell its rounded axis estimate names? Rows the host does not
// hold (device sources, staged rows) count as cells: the planners append grid cells.
static bool rows_on_cells(const mfgp_model* m, const GPDesc& d) {
  const GridLattice& L = m->lat;
  if (L.nx <= 0) return false;
  if (!d.rows_inline || d.k_new != d.N - d.n0 || (int)m->hax.size() != L.nx || (int)m->hay.size() != L.ny) return true;
  for (int64_t a = 0; a < d.k_new; ++a) {
    const double px = d.rows_xy[2 * a], py = d.rows_xy[2 * a + 1];
    if (!(px == px) || !(py == py)) return false;
    const int ix = (int)std::rint(std::fmin(std::fmax((px - L.x0) * L.xinv, 0.0), (double)(L.nx - 1)));
    const int iy = (int)std::rint(std::fmin(std::fmax((py - L.y0) * L.yinv, 0.0), (double)(L.ny - 1)));
    if (!(m->hax[ix] == px && m->hay[iy] == py)) return false;
  }
  return true;
}

// Enqueue assembly + blocked Cholesky for `count` models (descriptors already uploaded).
int enqueue_factor(mfgp_ctx* c, const GPDesc* dd, const GPDesc* hd, int count) {
  int64_t max_nb = 0, max_tiles = 0;
  for (int i = 0; i < count; ++i) {
    const int64_t nb = nblocks_factor(hd[i].N);
    max_nb = std::max(max_nb, nb);
    max_tiles = std::max(max_tiles, nb * (nb + 1) / 2);
  }
  EvPair ev{};
  int rc = ev_begin(c, ev, 1);
  if (rc) return rc;
  HIP_TRY(launch_assemble(dd, count, max_tiles, c->stream));
  // Blocked right-looking Cholesky, per 64-column step: diagonal factor +
  // inverse (k_potrf_diag), panel (k_panel), trailing update. Two-level: the
  // steps of a group of FD (c->factor_depth) update only the group's own columns
  // (k_syrk_blk, one step deep), and the rest of the trailing matrix takes the
  // group's FD steps in one pass (k_syrk_blk, FD deep) -- bit-equal to the
  // one-level order, each trailing tile read and written once per group.
  const int FD = std::max(1, c->factor_depth);
  hipStream_t cs = c->stream;
  for (int64_t K0 = 0; K0 < max_nb; K0 += FD) {
    const int64_t K1 = std::min<int64_t>(K0 + FD, max_nb);
    for (int64_t kb = K0; kb < K1; ++kb) {
      HIP_TRY(launch_potrf_diag(dd, count, (int)kb, cs));
      const int64_t below = max_nb - kb - 1;
      if (below <= 0) continue;
      HIP_TRY(launch_panel(dd, count, (int)kb, below, cs));
      const int64_t jmax = std::min<int64_t>(K0 + FD - 1, max_nb - 1);
      if (FD == 1) {
        HIP_TRY(launch_syrk(dd, count, (int)kb, below * (below + 1) / 2, 0, cs));
      } else if (jmax >= kb + 1) {
        int64_t tiles = 0;
        for (int64_t j = kb + 1; j <= jmax; ++j) tiles += max_nb - j;
        HIP_TRY(launch_syrk_blk(dd, count, (int)kb, 1, (int)(kb + 1), (int)jmax, tiles, cs));
      }
    }
    const int64_t jmin = K0 + FD;
    if (FD > 1 && jmin < max_nb) {
      const int64_t T = max_nb - jmin;
      HIP_TRY(launch_syrk_blk(dd, count, (int)K0, (int)(K1 - K0), (int)jmin, INT32_MAX, T * (T + 1) / 2, cs));
    }
  }
  int64_t max_n = 0;
  for (int i = 0; i < count; ++i) max_n = std::max(max_n, hd[i].N);
  HIP_TRY(launch_extract_z(dd, count, max_n, c->stream));
  return ev_end(c, ev);
}

static int enqueue_inc_factor(mfgp_ctx* c, const GPDesc* dd, const GPDesc* hd, int count) {
  int64_t max_np = 0;
  for (int i = 0; i < count; ++i) max_np = std::max<int64_t>(max_np, hd[i].nprod);
  EvPair ev{};
  int rc = ev_begin(c, ev, 1);
  if (rc) return rc;
  HIP_TRY(launch_inc_stream(dd, count, max_np, hd[0].vf32, c->stream));
  return ev_end(c, ev);
}

int enqueue_vstream(mfgp_ctx* c, const GPDesc* dd, const GPDesc* hd, int count) {
  int64_t max_ct = 0;
  for (int i = 0; i < count; ++i) max_ct = std::max(max_ct, ntiles_wg(hd[i].M, hd[i].rsplit, hd[i].vf32));
  if (max_ct == 0) return MFGP_OK;
  EvPair ev{};
  int rc = ev_begin(c, ev, 0);
  if (rc) return rc;
  HIP_TRY(launch_vstream(dd, count, max_ct, hd[0].vf32, c->stream));
  return ev_end(c, ev);
}

// fp64 V bytes of a full predict of descriptor d (k_predict's image of V).
static size_t v64_bytes(const GPDesc& d) { return sizeof(double) * (size_t)ntiles_grid(d.M) * d.vld * PBM; }

// MFGP_F32 full predicts compute V in fp64 scratch (k_predict's left-looking
// solve re-reads its own rows) and round it into the resident fp32 V
// (k_vnarrow): point the descriptors at slots of the context's scratch, as many
// GPs per launch as F32_SCRATCH holds (at least one). Call before the upload.
int assign_predict_scratch(mfgp_ctx* c, GPDesc* hd, int count) {
  if (count <= 0 || !hd[0].vf32) return MFGP_OK;
  size_t per = 0;
  for (int i = 0; i < count; ++i) per = std::max(per, v64_bytes(hd[i]));
  per = WsLayout::up(per);
  if (per == 0) return MFGP_OK;
  int g = (int)std::max<size_t>(1, std::min<size_t>((size_t)count, F32_SCRATCH / per));
  if (per * g > c->vscr.bytes()) {
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->vscr.reset();
    // at most half of the free HBM (the resident state of the models comes first);
    // mfgp_ctx_trim gives the scratch back
    size_t fr = 0, tot = 0;
    if (hipMemGetInfo(&fr, &tot) == hipSuccess && per * g > fr / 2)
      g = (int)std::max<size_t>(1, std::min<size_t>((size_t)g, fr / 2 / per));
    if (const int rc = dev_alloc(c->vscr, c->stream, per * g, A_NO_DRAIN)) return rc;
  }
  c->f32_group = g;
  for (int i = 0; i < count; ++i) hd[i].V = c->vscr + (per / sizeof(double)) * (i % g);
  return MFGP_OK;
}

int enqueue_predict(mfgp_ctx* c, const GPDesc* dd, const GPDesc* hd, int count) {
  int64_t max_ct = 0;
  for (int i = 0; i < count; ++i) {
    max_ct = std::max(max_ct, ntiles_grid(hd[i].M));
    // k_predict addresses A through a 32-bit buffer descriptor: 8 * ld^2 < 2^31
    if (hd[i].ld > MAX_FULL_CAP + 64)
      return set_err(MFGP_ERR_ARG,
                     "the full predict supports a training capacity of at most %lld rows (this model's is %lld, N = %lld)",
                     (long long)MAX_FULL_CAP, (long long)(hd[i].ld - 1), (long long)hd[i].N);
  }
  if (max_ct == 0) return MFGP_OK;
  EvPair ev{};
  int rc = ev_begin(c, ev, 0);
  if (rc) return rc;
  if (!hd[0].vf32) {
    HIP_TRY(launch_predict(dd, count, max_ct, c->stream));
  } else {
    // groups sharing the scratch run one after the other (stream order)
    const int g = c->f32_group;
    for (int g0 = 0; g0 < count; g0 += g) {
      const int gn = std::min(g, count - g0);
      HIP_TRY(launch_predict(dd + g0, gn, max_ct, c->stream));
      HIP_TRY(launch_vnarrow(dd + g0, gn, max_ct, c->stream));
    }
  }
  return ev_end(c, ev);
}

// bytes of T scratch the recursive-doubling F build may hold in the workspace
constexpr int64_t TRINV_WS_MAX = int64_t(2) << 30;

static int ensure_sync(mfgp_model* m) {
  if (m->sync) return MFGP_OK;
  return dev_alloc(m->sync, m->ctx->stream, 4 * sizeof(unsigned), A_ZERO | A_NO_DRAIN);
}

// Bordered appends and their one-pass predicts in one k_inc_stream launch (dd == null:
// the host descriptors by value, k_inc_stream_arg).
static int enqueue_inc_stream(mfgp_ctx* c, const GPDesc* dd, const GPDesc* hd, int count) {
  int64_t max_blocks = 0;
  for (int i = 0; i < count; ++i)
    max_blocks = std::max(max_blocks, hd[i].nprod + ntiles_wg(hd[i].M, hd[i].rsplit, hd[i].vf32));
  EvPair ev{};
  int rc = ev_begin(c, ev, 0);
  if (rc) return rc;
  HIP_TRY(dd ? launch_inc_stream(dd, count, max_blocks, hd[0].vf32, c->stream)
             : launch_inc_stream_arg(hd, count, max_blocks, hd[0].vf32, c->stream));
  return ev_end(c, ev);
}

// Lattice-separable appends + predicts (k_inc_lat), after the explicit inverses
// and the separable tables they need (k_trinv_f / k_lat_tables: only when a model
// enters the mode with a new factor, grid or hyperparameters).
static int enqueue_inc_lat(mfgp_ctx* c, const GPDesc* dd, const GPDesc* hd, int count) {
  int64_t max_blocks = 0, max_nbr = 0, max_rows = 0, max_axw = 0, max_tiles = 0, max_vcr = 0, max_vct = 0;
  for (int i = 0; i < count; ++i) {
    if (hd[i].vcol && hd[i].vcol_lo < hd[i].n0) {
      max_vcr = std::max(max_vcr, hd[i].n0 - hd[i].vcol_lo);
      max_vct = std::max(max_vct, ntiles_grid(hd[i].M));
    }
    max_blocks = std::max<int64_t>(max_blocks, hd[i].nprod + hd[i].nwu + hd[i].nzu + (hd[i].lat_zcsr ? 2 : 0) +
                                                   (hd[i].lat_g2 ? 0 : (int64_t)hd[i].lat_tiles * hd[i].ksplit));
    max_tiles = std::max<int64_t>(max_tiles, hd[i].lat_tiles);
    if (hd[i].lat_fbuild) max_nbr = std::max(max_nbr, nblocks_rows(hd[i].n0));
    max_rows = std::max(max_rows, hd[i].n0 - hd[i].tab_lo);
    if (hd[i].lat_axbuild) max_axw = std::max(max_axw, hd[i].tabw);
  }
  // the builds a new factor / grid / hyperparameters need, timed as factor work
  // (mfgp_ctx_get_timing's factor counters)
  EvPair evb{};
  if (max_nbr > 0 || max_rows > 0 || max_axw > 0 || max_vcr > 0) {
    int rc = ev_begin(c, evb, 1);
    if (rc) return rc;
  }
  if (max_nbr > 0) {
    // recursive doubling needs a T scratch per GP (8 MB at n0 = 2048); MFGP_TRINV_COLUMNS=1:
    // the block-column form (diagnostics)
    const int64_t tstride = trinv_scratch(max_nbr);
    double* tscr = nullptr;
    // the scratch is bounded (TRINV_WS_MAX, and half the free HBM): a batch that needs
    // more runs in GP chunks (configs[4]: 32 GPs x 128 MiB at N = 8192 -> chunks of 8)
    int chunk = count;
    if (!c->trinv_columns) {
      size_t free_b = 0, total_b = 0;
      int64_t budget = TRINV_WS_MAX;
      if (hipMemGetInfo(&free_b, &total_b) == hipSuccess)
        budget = std::min<int64_t>(budget, (int64_t)((free_b + c->ws.bytes()) / 2));
      const int64_t per_gp = (int64_t)sizeof(double) * tstride;
      chunk = (int)std::max<int64_t>(1, std::min<int64_t>(count, budget / std::max<int64_t>(per_gp, 1)));
      int rc = ensure_ws(c, sizeof(double) * (size_t)(tstride * chunk));
      if (rc) return rc;
      tscr = c->ws;
    }
    for (int i0 = 0; i0 < count; i0 += chunk)
      HIP_TRY(launch_trinv_f(dd + i0, std::min(chunk, count - i0), max_nbr, tscr, tstride, c->stream));
    // MFGP_F32: the copy the lattice step streams, rounded once per build
    if (hd[0].vf32) {
      int64_t max_el = 0;
      for (int i = 0; i < count; ++i)
        if (hd[i].lat_fbuild) max_el = std::max<int64_t>(max_el, fblk_size(hd[i].ld));
      HIP_TRY(launch_narrow_f(dd, count, max_el, c->stream));
    }
  }
  if (max_rows > 0) HIP_TRY(launch_lat_tables(dd, count, max_rows, c->stream));
  if (max_axw > 0) HIP_TRY(launch_lat_axes(dd, count, max_axw, c->stream));
  // the column stores that are behind V (a new factor, V-stream steps since): caught up
  if (max_vcr > 0) HIP_TRY(launch_vcol_build(dd, count, max_vcr, max_vct, hd[0].vf32, c->stream));
  {
    int rc = ev_end(c, evb);
    if (rc) return rc;
  }
  EvPair ev{};
  int rc = ev_begin(c, ev, 0);
  if (rc) return rc;
  // (dd == null: the host descriptors by value; desc_arg_ok: none of the builds above ran)
  const int ka = hd[0].ka, vf = hd[0].vf32;
  HIP_TRY(dd ? launch_inc_lat(dd, count, max_blocks, ka, vf, !hd[0].lat_g2, c->stream)
             : launch_inc_lat_arg(hd, count, max_blocks, ka, vf, !hd[0].lat_g2, c->stream));
  if (hd[0].lat_g2)
    HIP_TRY(dd ? launch_lat_gemm2(dd, count, max_tiles, ka, vf, c->stream)
               : launch_lat_gemm2_arg(hd, count, max_tiles, ka, vf, c->stream));
  return ev_end(c, ev);
}

// A batch step that is one launch takes its host descriptors by value
// (k_inc_stream_arg, k_inc_lat_arg). The lattice step alone (k_inc_lat_arg):
// for a batch step that needs nothing else on the device -- no F / table / axis
// builds, no other appends or predicts -- so the descriptor array is not uploaded.
static bool desc_arg_ok(const mfgp_ctx* c, const GPDesc* hd, int count) {
  if (!c->desc_arg || count < 1 || count > DESC_ARG_MAX) return false;
  for (int i = 0; i < count; ++i)
    if (hd[i].lat_fbuild || hd[i].n0 > hd[i].tab_lo || hd[i].lat_axbuild || (hd[i].vcol && hd[i].vcol_lo < hd[i].n0))
      return false;
  return true;
}

// Row splits of the one-pass predict for a launch over these descriptors: 128-cell
// workgroups while they fill the chip (~4 per CU), else 64 or 32 cells with the
// rows split 2 or 4 ways (the drop-in simulator predicts one GP at a time).
void set_rsplit(const mfgp_ctx* c, GPDesc* hd, int count) {
  if (count > 0 && hd[0].vf32) {   // the fp32 stream has no row splits
    for (int i = 0; i < count; ++i) hd[i].rsplit = 1;
    return;
  }
  int64_t w1 = 0;
  for (int i = 0; i < count; ++i) w1 += ntiles_wg(hd[i].M);
  int R = (w1 >= 3 * c->ncu) ? 1 : (2 * w1 >= 3 * c->ncu ? 2 : 4);
  if (c->rsplit_force > 0) R = c->rsplit_force;   // (diagnostics: MFGP_RSPLIT)
  for (int i = 0; i < count; ++i) hd[i].rsplit = R;
}

static void mark_full_factor(mfgp_model* m) {
  m->cnt[N_FULL_FACTOR] += 1;
  const int64_t N = m->NL + m->NH;
  m->st.full_factor_enqueued(N, nblocks_factor(N), m->hyp, m->jitter);
}

void mark_inc_factor(mfgp_model* m) {
  m->cnt[N_INC_FACTOR] += 1;
  const int64_t N = m->NL + m->NH;
  m->st.inc_factor_enqueued(N, nblocks_factor(N));
}

// Descriptor of a bordered append of rows [factor_N, N) (k_inc_stream; the
// caller sets tiles = 1 and the predict outputs to stream the cells too).
int fill_inc_desc(GPDesc& d, mfgp_model* m) {
  int rc = ensure_sync(m);
  if (rc) return rc;
  fill_desc(d, m);
  d.n0 = m->st.factor_N;
  d.vres = m->V ? m->st.v_n : 0;
  d.sync = m->sync;
  if (++m->epoch == 0) m->epoch = 1;
  d.epoch = m->epoch;
  d.nprod = (int)fused_producers(d.n0);
  d.l21c_ok = 1;   // the producers write the compact rows for (n0, N)
  m->st.compact_rows_written(d.n0, d.N);
  return MFGP_OK;
}

// One-pass predict over the V rows [0, v_n): the compact rows serve it when the
// last bordered append wrote them for exactly these rows.
void set_vstream_rows(GPDesc& d, const mfgp_model* m) {
  d.n0 = m->st.v_n;
  d.l21c_ok = m->st.l21c_ok(m->NL + m->NH) ? 1 : 0;
}

// Factor one model now (synchronous, status checked).
int factor_one(mfgp_model* m) {
  mfgp_ctx* c = m->ctx;
  int rc = ensure_cap(m, m->NL + m->NH);
  if (rc) return rc;
  int slot;
  GPDesc* hd = acquire_slot(c, slot, rc);
  if (!hd) return rc;
  fill_desc(hd[0], m);
  const GPDesc* dd = nullptr;
  if ((rc = upload_slot(c, slot, 1, &dd))) return rc;
  if ((rc = enqueue_factor(c, dd, hd, 1))) return rc;
  if ((rc = release_slot(c, slot))) return rc;
  HIP_TRY(hipStreamSynchronize(c->stream));
  mark_full_factor(m);
  rc = read_status(m);
  m->st.factor_checked(rc == MFGP_OK);
  return rc;
}

// Bring the factor up to date for all N rows: bordered append of the rows
// beyond factor_N when possible, else a full refactor (synchronous).
int update_factor(mfgp_model* m) {
  if (factor_current(m)) return MFGP_OK;
  if (!can_inc_factor(m)) return factor_one(m);
  mfgp_ctx* c = m->ctx;
  int rc, slot;
  GPDesc* hd = acquire_slot(c, slot, rc);
  if (!hd) return rc;
  if ((rc = fill_inc_desc(hd[0], m))) return rc;
  const GPDesc* dd = nullptr;
  if ((rc = upload_slot(c, slot, 1, &dd))) return rc;
  if ((rc = enqueue_inc_factor(c, dd, hd, 1))) return rc;
  if ((rc = release_slot(c, slot))) return rc;
  HIP_TRY(hipStreamSynchronize(c->stream));
  mark_inc_factor(m);
  rc = read_status(m);
  m->st.factor_checked(rc == MFGP_OK);
  return rc;
}

// ---- the lattice step's plan for one sub-batch (mfgp_lat_plan.h has the arithmetic) ----
struct LatPlan {
  bool take = false;    // the step is taken (eligible for every member, and cheaper than the V stream)
  int ka = 8;
  bool g2 = false;      // the GEMM and cells as a second launch (k_lat_gemm2), else in-launch tiles
  int ksplit = 1;       // split-K of the in-launch tiles
  int64_t wu_total = 0;
  int nwu[MAXB / 2];    // each member's w units
  int selfg = 0;        // w units gather L21 from V themselves
  bool vcol_all = false;   // every member has a column store: the w units read it
};

// lattice grids, well-conditioned K and a resident posterior of the old rows:
// the separable step (k_inc_lat) instead of the V stream. order / hd: the ninc
// bordered appends of a fused sub-batch and their descriptors.
static int plan_lat(mfgp_ctx* c, mfgp_model* const* order, const GPDesc* hd, int ninc, LatPlan& p) {
  for (int i = 0; i < ninc; ++i)
    if (!lat_eligible(order[i], hd[i].n0)) return MFGP_OK;
  mfgp_lat_plan::Gp g[MAXB / 2];
  for (int i = 0; i < ninc; ++i) {
    const mfgp_model* m = order[i];
    g[i] = {hd[i].n0, m->NL + m->NH - hd[i].n0, m->M, m->dtype == MFGP_F32 ? 4 : 8, m->lat.nx, m->lat.ny,
            m->kind == MFGP_SF};
  }
  const mfgp_lat_plan::Knobs kn = {c->ncu, c->lat_gemm2, c->concurrent, c->lat_force, c->lat_ksplit, c->lat_wu};
  const mfgp_lat_plan::Plan q = mfgp_lat_plan::plan(kn, g, ninc);
  if (!q.take) return MFGP_OK;
  p.ka = q.ka;
  p.g2 = q.g2;
  p.ksplit = q.ksplit;
  p.wu_total = q.wu_total;
  for (int i = 0; i < ninc; ++i) p.nwu[i] = mfgp_lat_plan::w_share(q.wu_total, q.wsteps_sum, hd[i].n0);

  // w units that gather L21 from V themselves start the F stream at once; each
  // row's gather is repeated in every block column it meets (~2x F's bytes in
  // cache lines), which a batch's concurrent streams pay for (B = 8: 101.7 vs
  // 99.5 us) and one GP does not (57.1 vs 60.3 us)
  p.selfg = c->lat_selfg >= 0 ? c->lat_selfg : (ninc == 1 ? 1 : 0);
  // the column store of V: taken by a batch whose models all have one (the w units
  // then start F at launch; one GP prefers it to the V self-gather). A model that
  // has a store keeps it written through whichever source the step reads
  p.vcol_all = c->lat_vcol != 0;
  for (int i = 0; i < ninc; ++i) {
    mfgp_model* m = order[i];
    if (c->lat_vcol != 0)
      if (const int rc = ensure_vcol(m)) return rc;
    p.vcol_all = p.vcol_all && m->Vc != nullptr && m->vc_ld == m->vld && m->vc_M == m->M;
  }
  p.take = true;
  return MFGP_OK;
}

// The lattice step's part of a bordered append's descriptor (after ensure_lat); returns
// the resident buffer the step reads (it writes the other).
static int fill_lat_desc(GPDesc& fd, mfgp_model* m, const LatPlan& p, int nwu, int64_t tiles, int64_t nzu) {
  const mfgp_ctx* c = m->ctx;
  const int ka = p.ka;
  const int bin = res_find(m, fd.n0);
  fd.rmu_in = res_mu(m, bin);
  fd.rvar_in = res_var(m, bin);
  fd.rmu = res_mu(m, 1 - bin);
  fd.rvar = res_var(m, 1 - bin);
  fd.F = m->F;
  fd.Ff = m->Ff;
  fd.tab = m->tab;
  fd.tabw = m->tabw;
  fd.wv = m->wv;
  fd.wflag = m->wflag;
  fd.gpart = m->gpart;
  fd.gcnt = m->gcnt;
  fd.ka = ka;
  fd.ksplit = p.ksplit;
  fd.lat_tiles = (int)tiles;
  fd.nwb = (int)((fd.n0 + 63) / 64);
  fd.nwu = nwu;
  fd.wpart = m->wpart;
  fd.wcnt = m->wcnt;
  fd.lat_fbuild = m->st.lat_fbuild(fd.n0) ? 1 : 0;
  fd.lidx = m->lidx;
  fd.axt = m->axt;
  fd.zb = m->zb;
  fd.zrows = m->zb_rows;
  fd.zflag = m->zflag;
  fd.ldone = m->ldone;
  fd.zvl = m->zvl;
  fd.nzu = (int)nzu;
  fd.zq = lat_zq(m);
  fd.lat_axbuild = m->st.lat_axbuild() ? 1 : 0;
  fd.lat_selfg = p.selfg;
  if (c->lat_vcol != 0 && m->Vc && m->vc_ld == m->vld && m->vc_M == m->M) {
    fd.vcol = m->Vc;
    fd.vcol_ld = m->vc_ld;
    // (the step's n0 rows of V are valid: fuse requires n0 == v_n)
    fd.vcol_lo = std::min(vcol_rows(m), fd.n0);
    fd.lat_vcol = p.vcol_all ? 1 : 0;
  }
  fd.lat_g2 = p.g2 ? 1 : 0;
  // Z units reading the scan units' member lists (every lattice row count the scan
  // units bucket, rows and lattice indices within 16 bits)
  // -- by default (the bucketing Z units scan every row of their part; with the
  // lists: headline 93.2k -> 95.3k GP-updates/s, configs[4] 17.8k -> 19.3k)
  const bool zc = c->lat_zcsr != 0;
  fd.lat_zcsr = (zc && ka == 8 && m->lat.ny <= 256 && m->ld <= 65535) ? 1 : 0;
  fd.csr = m->csr;
  fd.tab_lo = m->st.tab_lo(fd.n0);
  return bin;
}

// The unchanged members of a batch step (batch_run's pre-pass).
// Members that append nothing to a current factor whose posterior is resident
// for its rows (the lockstep simulations: seeds whose agents all exploited this
// iteration, sim:872-891) are unchanged: their predict is the resident posterior,
// copied into the outputs with its var max / argmax (k_post_copy, one launch),
// and the batch step runs over the others -- so a ragged batch keeps its one
// fused (or lattice) launch instead of falling back to streaming V for all.
// *served: there were such members and the whole step ran from here (the result is
// returned); else nothing was done and batch_run goes on over all members.
static int serve_unchanged(mfgp_model** models, int count, const double* X, const double* y, const int64_t* k,
                           double* mu, double* var, double* vmax, int64_t* vargmax, int flags, bool* served) {
  mfgp_ctx* c = models[0]->ctx;
  const bool rows_given = k && X && y;
  bool any_unchanged = false;   // (cheap test first: the pointer queries cost ~1 us each)
  for (int i = 0; i < count && !any_unchanged; ++i) any_unchanged = !rows_given || k[i] == 0;
  if (!any_unchanged || !is_device_ptr(mu) || !is_device_ptr(var)) return MFGP_OK;
  std::vector<PostCopy> pc;
  std::vector<mfgp_model*> rest;
  std::vector<int64_t> rest_k, rest_off;
  std::vector<int> rest_vidx;
  int64_t oo = 0;
  for (int i = 0; i < count; ++i) {
    mfgp_model* m = models[i];
    const int64_t ki = rows_given ? k[i] : 0;
    const int64_t n = m->NL + m->NH;
    const int b = (ki == 0 && m->M > 0 && factor_current(m) && m->st.v_n == n) ? res_find(m, n) : -1;
    if (b >= 0) {
      pc.push_back({res_mu(m, b), res_var(m, b), mu + oo, var + oo, vmax ? vmax + i : nullptr,
                    vargmax ? vargmax + i : nullptr, m->M});
      m->cnt[N_POST_COPY] += 1;
    } else {
      rest.push_back(m);
      rest_k.push_back(ki);
      rest_off.push_back(oo);
      rest_vidx.push_back(i);
    }
    oo += m->M;
  }
  if (pc.empty()) return MFGP_OK;
  *served = true;
  HIP_TRY(launch_post_copy(pc.data(), (int)pc.size(), c->stream));
  if (rest.empty()) return (flags & MFGP_ASYNC) ? MFGP_OK : mfgp_ctx_synchronize(c);
  // (the rows of the unchanged members are none: the others' rows stay contiguous)
  return batch_run(rest.data(), (int)rest.size(), X, y, rest_k.data(), mu, var, vmax, vargmax, flags, true, true,
                   rest_off.data(), rest_vidx.data());
}

// One call of batch_run: its arguments, its members' offsets into the new rows and the
// outputs, and the vectors its sub-batches reuse.
struct BatchCall {
  mfgp_ctx* c;
  mfgp_model** models;
  const double *X, *y;
  const int64_t* k;
  double *mu, *var, *vmax;
  int64_t* vargmax;
  const int* vidx;
  bool do_factor, do_predict;
  bool has_new, dev_src;   // rows are appended; from device memory
  std::vector<int64_t> src_off, out_off, oo_ord;
  std::vector<mfgp_model*> order, porder;
  // per predict of a sub-batch: the resident buffer it writes (-1: none) and, for a lattice
  // step, that buffer's depth
  int res_b[MAXB / 2], res_depth[MAXB / 2];
  int fill_factor_descs(int b0, int nb, GPDesc* hd, int& ninc, int& nfull);
  void note_predicts(int np, int nv, int nlat, const GPDesc* hd, bool lat_arg, bool g2);
  int sub_batch(int b0, int nb);
};

// factor descriptors, ordered [bordered appends | full refactors | current]:
// the factor kernels run over their contiguous sub-ranges (k_inc_l21 lands
// the device-resident rows of the bordered appends, k_append those of the
// full refactors)
int BatchCall::fill_factor_descs(int b0, int nb, GPDesc* hd, int& ninc, int& nfull) {
  int rc;
  for (int i = 0; i < nb; ++i)
    if (!factor_current(models[b0 + i]) && can_inc_factor(models[b0 + i])) order.push_back(models[b0 + i]);
  ninc = (int)order.size();
  for (int i = 0; i < nb; ++i)
    if (!factor_current(models[b0 + i]) && !can_inc_factor(models[b0 + i])) order.push_back(models[b0 + i]);
  nfull = (int)order.size() - ninc;
  for (int i = 0; i < nb; ++i)
    if (factor_current(models[b0 + i])) order.push_back(models[b0 + i]);
  for (int i = 0; i < nb; ++i) {
    mfgp_model* m = order[i];
    if (i < ninc) {
      if ((rc = fill_inc_desc(hd[i], m))) return rc;
    } else {
      fill_desc(hd[i], m);
    }
    const int mi = (int)(std::find(models + b0, models + b0 + nb, m) - models);
    const int64_t ki = has_new ? k[mi] : 0;
    if (ki <= 0) continue;
    if (dev_src) {
      hd[i].srcX = X + 2 * src_off[mi];
      hd[i].srcY = y + src_off[mi];
      hd[i].k_new = ki;
    } else if (i < ninc && ki <= KINC) {
      std::memcpy(hd[i].rows_xy, X + 2 * src_off[mi], sizeof(double) * 2 * ki);
      std::memcpy(hd[i].rows_y, y + src_off[mi], sizeof(double) * ki);
      hd[i].rows_inline = 1;
      hd[i].k_new = ki;
    } else if ((rc = copy_rows(m, m->NL + m->NH - ki, X + 2 * src_off[mi], y + src_off[mi], ki))) {
      return rc;
    }
  }
  for (int i = 0; i < ninc + nfull; ++i) {   // host bookkeeping of the factors enqueued below
    if (i < ninc) mark_inc_factor(order[i]);
    else mark_full_factor(order[i]);
    add_async_status(c, order[i]);
  }
  return MFGP_OK;
}

// The step of one GP publishes its status into a mapped word of the model (and the
// L22 verdict into a second one): the words reset, the descriptor pointed at them and
// the model's deferred status entry told to read the word.
static int publish_mapped_status(mfgp_ctx* c, mfgp_model* m, GPDesc& d) {
  if (!m->status_host) {
    int rc;
    if ((rc = pin_alloc(m->status_host, 2 * sizeof(int), hipHostMallocMapped))) return rc;
    if ((rc = pin_device(m->status_host, m->status_host_dev))) {
      m->status_host.reset();
      return rc;
    }
  }
  volatile int* const words = m->status_host.get();
  words[0] = STATUS_UNSET;
  words[1] = STATUS_UNSET;
  d.status_host = m->status_host_dev;
  d.pd_host = m->status_host_dev + 1;
  for (auto it = c->async_status.rbegin(); it != c->async_status.rend(); ++it)
    if (it->m == m) {
      it->host = m->status_host;
      break;
    }
  return MFGP_OK;
}

// The host bookkeeping of the predicts enqueued (porder: nv one-pass predicts, then
// full ones), of which the first nlat ran as lattice steps over the descriptors hd.
void BatchCall::note_predicts(int np, int nv, int nlat, const GPDesc* hd, bool lat_arg, bool g2) {
  for (int i = 0; i < np; ++i) {
    mfgp_model* m = porder[i];
    const Predict kind = i < nlat ? Predict::Lattice : (i < nv ? Predict::VStream : Predict::Full);
    m->st.predict_enqueued(kind, m->NL + m->NH, res_b[i], i < nlat ? res_depth[i] : 0, i < nlat && hd[i].vcol);
    (i < nv ? m->cnt[N_VSTREAM] : m->cnt[N_FULL_PREDICT]) += 1;
    if (i < nlat) {
      m->cnt[N_LATTICE] += 1;
      if (lat_arg) m->cnt[N_LATTICE_ARG] += 1;
      if (g2) m->cnt[N_LATTICE_G2] += 1;
      if (hd[i].vcol) {   // caught up to n0 ahead of the step, the new rows written through
        m->cnt[N_VCOL_ROWS] += hd[i].n0 - hd[i].vcol_lo;
        m->cnt[N_LATTICE_VCOL] += (hd[i].lat_vcol && rows_on_cells(m, hd[i])) ? 1 : 0;
      }
    }
  }
}

// One sub-batch of a batch step: members [b0, b0 + nb) through one descriptor slot,
// [factor order | predict order].
int BatchCall::sub_batch(int b0, int nb) {
  int rc = MFGP_OK;
  if (do_predict) {
    for (int i = 0; i < nb; ++i)
      if (models[b0 + i]->M > 0 && (rc = ensure_v(models[b0 + i]))) return rc;
  }
  int slot;
  GPDesc* hd = acquire_slot(c, slot, rc);
  if (!hd) return rc;
  int ninc = 0, nfull = 0;
  order.clear();
  if (do_factor && (rc = fill_factor_descs(b0, nb, hd, ninc, nfull))) return rc;
  // predict descriptors (state after the factor step), ordered
  // [one-pass predicts over resident V | full predicts]
  int nv = 0, np = 0;
  if (do_predict) {
    porder.clear();
    oo_ord.clear();
    for (int pass = 0; pass < 2; ++pass)
      for (int i = 0; i < nb; ++i) {
        mfgp_model* m = models[b0 + i];
        if (m->M == 0 || can_vstream(m) != (pass == 0)) continue;
        porder.push_back(m);
        oo_ord.push_back(out_off[b0 + i]);
      }
    np = (int)porder.size();
    while (nv < np && can_vstream(porder[nv])) ++nv;
    for (int i = 0; i < np; ++i) {
      GPDesc& pd = hd[nb + i];
      fill_desc(pd, porder[i]);
      res_b[i] = set_res_out(porder[i], pd, -1);
      if (i < nv) set_vstream_rows(pd, porder[i]);
      pd.mu = mu + oo_ord[i];
      pd.var = var + oo_ord[i];
      int64_t mi = std::find(models + b0, models + b0 + nb, porder[i]) - models;
      if (vidx) mi = vidx[mi];
      if (vmax) pd.vmax = vmax + mi;
      if (vargmax) pd.vargmax = vargmax + mi;
    }
  }
  // bordered appends whose one-pass predicts follow from the same rows (V
  // resident up to the old factor) run as one k_inc_stream launch: their
  // factor descriptors take the predict outputs and the hand-off state
  bool fuse = c->fused && ninc > 0 && ninc == nv;
  for (int i = 0; fuse && i < ninc; ++i) fuse = order[i] == porder[i] && hd[i].n0 == porder[i]->st.v_n;
  if (fuse) {
    for (int i = 0; i < ninc; ++i) {
      GPDesc& fd = hd[i];
      const GPDesc& pd = hd[nb + i];
      fd.mu = pd.mu;
      fd.var = pd.var;
      fd.vmax = pd.vmax;
      fd.vargmax = pd.vargmax;
      fd.rmu = pd.rmu;
      fd.rvar = pd.rvar;
      fd.tiles = 1;
    }
  }
  LatPlan lp;
  if (fuse && (rc = plan_lat(c, order.data(), hd, ninc, lp))) return rc;
  const bool lat = lp.take, g2 = lat && lp.g2;
  for (int i = 0; lat && i < ninc; ++i) {
    mfgp_model* m = order[i];
    const int64_t tiles = g2 ? mfgp_lat_plan::tiles2(m->lat.nx, m->lat.ny, lp.ka)
                             : mfgp_lat_plan::tiles(m->lat.nx, m->lat.ny, lp.ka);
    const int64_t nzu = lat_nzu(m);
    if ((rc = ensure_lat(m, tiles, lp.ksplit, lp.ka, nzu))) return rc;
    const int bin = fill_lat_desc(hd[i], m, lp, lp.nwu[i], tiles, nzu);
    res_b[i] = 1 - bin;
    res_depth[i] = m->st.res[bin].depth + 1;
  }
  if (nv > 0) {
    set_rsplit(c, hd + nb, nv);
    for (int i = 0; fuse && i < ninc; ++i) hd[i].rsplit = hd[nb].rsplit;
  }
  if (np > nv && (rc = assign_predict_scratch(c, hd + nb + nv, np - nv))) return rc;
  // one GP, append + one-pass predict fused, nothing else: launch with the
  // descriptor by value (no upload) and the status published into a mapped word
  // (the lattice step of one GP publishes its status the same way)
  const bool single = fuse && nb == 1 && ninc == 1 && np == 1 && nv == 1;
  if (single && (rc = publish_mapped_status(c, order[0], hd[0]))) return rc;
  if (single && !lat) {
    mfgp_model* m = order[0];
    EvPair ev{};
    if ((rc = ev_begin(c, ev, 0))) return rc;
    HIP_TRY(launch_inc_stream1(hd[0], hd[0].nprod + ntiles_wg(hd[0].M, hd[0].rsplit, hd[0].vf32), hd[0].vf32,
                               c->stream));
    if ((rc = ev_end(c, ev))) return rc;
    release_slot_unread(c, slot);
    m->st.predict_enqueued(Predict::VStream, m->NL + m->NH, res_b[0]);
    m->cnt[N_VSTREAM] += 1;
    return MFGP_OK;
  }
  bool lat_arg = false, by_value = false;
  if (do_factor && lat && nfull == 0 && ninc == nb && np == nv && desc_arg_ok(c, hd, ninc)) {
    // the whole step is one k_inc_lat launch: its descriptors go by value
    if ((rc = enqueue_inc_lat(c, nullptr, hd, ninc))) return rc;
    lat_arg = by_value = true;
  } else if (do_factor && fuse && !lat && nfull == 0 && ninc == nb && np == nv && c->desc_arg &&
             ninc <= DESC_ARG_MAX) {
    // the whole step is one k_inc_stream launch (append + one-pass predict)
    if ((rc = enqueue_inc_stream(c, nullptr, hd, ninc))) return rc;
    by_value = true;
  } else {
  const GPDesc* dd = nullptr;
  if ((rc = upload_slot(c, slot, nb + np, &dd))) return rc;
  if (do_factor) {
    if (dev_src && nfull > 0) HIP_TRY(launch_append(dd + ninc, nfull, c->stream));
    if (ninc > 0 && (rc = lat ? enqueue_inc_lat(c, dd, hd, ninc)
                              : (fuse ? enqueue_inc_stream(c, dd, hd, ninc) : enqueue_inc_factor(c, dd, hd, ninc))))
      return rc;
    if (nfull > 0 && (rc = enqueue_factor(c, dd + ninc, hd + ninc, nfull))) return rc;
  }
  if (nv > 0 && !fuse && (rc = enqueue_vstream(c, dd + nb, hd + nb, nv))) return rc;
  if (np > nv && (rc = enqueue_predict(c, dd + nb + nv, hd + nb + nv, np - nv))) return rc;
  }
  if (by_value) {
    release_slot_unread(c, slot);
  } else if ((rc = release_slot(c, slot))) {
    return rc;
  }
  note_predicts(np, nv, lat ? ninc : 0, hd, lat_arg, g2);
  return MFGP_OK;
}

// Shared driver of the batched entry points: append (optional), factor
// (do_factor) and predict (do_predict) `count` models with one set of launches
// per kind: bordered appends (k_inc_factor) and full refactors side by side,
// then one-pass predicts over the resident V (k_vstream) and full predicts.
// out_offs / vidx (or null): each model's offset into mu / var and index into
// vmax / vargmax, when `models` is a subset of the caller's batch (the models left
// after the unchanged ones took k_post_copy)
int batch_run(mfgp_model** models, int count, const double* X, const double* y, const int64_t* k, double* mu,
              double* var, double* vmax, int64_t* vargmax, int flags, bool do_factor, bool do_predict,
              const int64_t* out_offs, const int* vidx) {
  if (!models || count <= 0) return set_err(MFGP_ERR_ARG, "empty batch");
  mfgp_ctx* c = models[0]->ctx;
  int rc = MFGP_OK;
  for (int i = 0; i < count; ++i) {
    if ((rc = check_model(models[i]))) return rc;
    if (models[i]->ctx != c) return set_err(MFGP_ERR_ARG, "batch models must share one context");
    if (models[i]->dtype != models[0]->dtype)
      return set_err(MFGP_ERR_ARG, "batch models must share one dtype (MFGP_F64 or MFGP_F32)");
    if (k && k[i] < 0) return set_err(MFGP_ERR_ARG, "negative k");
    if (!do_factor && !factor_current(models[i]))
      return set_err(MFGP_ERR_ARG, "model %d has no current factor (call mfgp_batch_append_factor first)", i);
  }
  if (do_predict && (!mu || !var)) return set_err(MFGP_ERR_ARG, "null output");
  if (do_factor && do_predict && !out_offs && c->incremental) {
    bool served = false;
    rc = serve_unchanged(models, count, X, y, k, mu, var, vmax, vargmax, flags, &served);
    if (served) return rc;
  }
  for (int i = 0; i < count; ++i) models[i]->spec_valid = false;
  // append new rows: device-resident sources are copied by one k_append launch
  // per sub-batch (below); host sources by plain copies here
  BatchCall q{c, models, X, y, k, mu, var, vmax, vargmax, vidx, do_factor, do_predict};
  const bool has_new = q.has_new = do_factor && k && X && y;
  q.dev_src = has_new && is_device_ptr(X) && is_device_ptr(y);
  std::vector<int64_t>&src_off = q.src_off, &out_off = q.out_off;
  src_off.assign(count, 0);
  out_off.assign(count, 0);
  int64_t off = 0, oo = 0;
  for (int i = 0; i < count; ++i) {
    mfgp_model* m = models[i];
    out_off[i] = out_offs ? out_offs[i] : oo;
    oo += m->M;
    if (!do_factor) continue;
    const int64_t ki = has_new ? k[i] : 0;
    const int64_t n = m->NL + m->NH;
    if ((rc = ensure_cap(m, n + ki))) return rc;
    src_off[i] = off;
    // host rows: the bordered appends carry them in their descriptors (rows_inline,
    // landed by the producers); the others are copied below, before their launches
    if (ki > 0) {
      m->NH += ki;
      bump_serial(m);
    }
    off += ki;
    if (!c->incremental) m->st.factor_lost(FactorLost::NotIncremental);   // reference behaviour: refactor every update
  }
  constexpr int CB = MAXB / 2;   // one descriptor slot per sub-batch: [factor order | predict order]
  for (int b0 = 0; b0 < count; b0 += CB)
    if ((rc = q.sub_batch(b0, std::min(CB, count - b0)))) return rc;
  if (flags & MFGP_ASYNC) return MFGP_OK;
  return mfgp_ctx_synchronize(c);
}
}  // namespace mfgp_host

extern "C" {

int mfgp_batch_truncate(mfgp_model** models, int count, int64_t n_keep_hifi) {
  const DeviceGuard dg_((models && count > 0 && models[0]) ? models[0]->ctx->device : -1);
  if (const int rc_ = settle((models && count > 0 && models[0]) ? models[0]->ctx : nullptr)) return rc_;
  if (count < 0 || (count > 0 && !models)) return set_err(MFGP_ERR_ARG, "bad batch");
  for (int i = 0; i < count; ++i) {
    const int rc = mfgp_truncate(models[i], n_keep_hifi);
    if (rc) return rc;
  }
  return MFGP_OK;
}

// The speculative form of an eager append (mfgp_append): the bordered append and
// the one-pass predict as one launch, synchronised (a non-PD step is reported
// here, as by update_factor), with mu | var kept for the next predict.
int spec_append_predict(mfgp_model* m, const double* X, const double* y, int64_t k) {
  mfgp_ctx* c = m->ctx;
  int rc = settle(c);
  if (rc == MFGP_OK) rc = ensure_spec_out(m);
  if (rc) return rc;
  if (m->status_host) static_cast<volatile int*>(m->status_host.get())[1] = STATUS_UNSET;
  // (the fused var max / argmax into the buffer's trailer: the launch's last cell
  // group reduces the groups' partials for the status word anyway)
  double* tr = m->spec_out_dev + 2 * m->spec_cap;
  m->spec_max = false;
  rc = batch_run(&m, 1, X, y, &k, m->spec_out_dev, m->spec_out_dev + m->spec_cap, tr,
                 reinterpret_cast<int64_t*>(tr + 1), MFGP_ASYNC, true, true);
  if (rc == MFGP_OK) m->spec_max = true;
  if (rc == MFGP_OK && c->early_pd && c->spin_us > 0 && m->status_host && c->async_status.size() == 1 &&
      c->async_status[0].host == m->status_host) {
    // the launch publishes the L22 verdict of the step (the only status its
    // factor can fail with) into the model's second mapped word: a positive
    // definite step returns now, and the next entry point settles the launch
    // (its outputs, hang guards) before anything reads or reuses its buffers
    const volatile int* w = static_cast<const volatile int*>(m->status_host.get()) + 1;
    const auto t0 = std::chrono::steady_clock::now();
    while (*w == STATUS_UNSET) {
      __builtin_ia32_pause();
      if (std::chrono::steady_clock::now() - t0 > std::chrono::microseconds(c->spin_us)) break;
    }
    if (*w == INT_MAX) {
      c->early_running = true;
      m->spec_valid = true;
      m->cnt[N_EARLY_PD] += 1;
      return MFGP_OK;
    }
  }
  if (rc == MFGP_OK) rc = mfgp_ctx_synchronize(c);
  if (rc != MFGP_OK) {
    m->st.factor_lost(FactorLost::StepFailed);   // a failed step leaves no usable factor
    return rc;
  }
  m->spec_valid = true;
  return MFGP_OK;
}

int mfgp_batch_append_predict(mfgp_model** models, int count, const double* X, const double* y, const int64_t* k,
                              double* mu, double* var, int flags) {
  const DeviceGuard dg_((models && count > 0 && models[0]) ? models[0]->ctx->device : -1);
  if (const int rc_ = settle((models && count > 0 && models[0]) ? models[0]->ctx : nullptr)) return rc_;
  return batch_run(models, count, X, y, k, mu, var, nullptr, nullptr, flags, true, true);
}

int mfgp_batch_append_predict_ex(mfgp_model** models, int count, const double* X, const double* y,
                                 const int64_t* k, double* mu, double* var, double* var_max, int64_t* var_argmax,
                                 int flags) {
  const DeviceGuard dg_((models && count > 0 && models[0]) ? models[0]->ctx->device : -1);
  if (const int rc_ = settle((models && count > 0 && models[0]) ? models[0]->ctx : nullptr)) return rc_;
  if ((var_max && !is_device_ptr(var_max)) || (var_argmax && !is_device_ptr(var_argmax)))
    return set_err(MFGP_ERR_ARG, "var_max / var_argmax must be device memory");
  return batch_run(models, count, X, y, k, mu, var, var_max, var_argmax, flags, true, true);
}

int mfgp_batch_append_factor(mfgp_model** models, int count, const double* X, const double* y, const int64_t* k,
                             int flags) {
  const DeviceGuard dg_((models && count > 0 && models[0]) ? models[0]->ctx->device : -1);
  if (const int rc_ = settle((models && count > 0 && models[0]) ? models[0]->ctx : nullptr)) return rc_;
  return batch_run(models, count, X, y, k, nullptr, nullptr, nullptr, nullptr, flags, true, false);
}

int mfgp_batch_predict(mfgp_model** models, int count, double* mu, double* var, int flags) {
  const DeviceGuard dg_((models && count > 0 && models[0]) ? models[0]->ctx->device : -1);
  if (const int rc_ = settle((models && count > 0 && models[0]) ? models[0]->ctx : nullptr)) return rc_;
  return batch_run(models, count, nullptr, nullptr, nullptr, mu, var, nullptr, nullptr, flags, false, true);
}

}  // extern "C"
