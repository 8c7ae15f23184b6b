// The planners of libmfgp_hip.so: the sample-point loops (mfgp_sample_points,
// mfgp_batch_sample_points) over the batch step, and the host side of the Voronoi-cell
// reductions (mfgp_cells.hip).
#include <chrono>
#include <cmath>
#include <cstring>

#include "mfgp_host.h"

using namespace mfgp;
using namespace mfgp_host;

extern "C" {

// The planners work on the caller's model itself instead of a deep copy (sim:339):
// the rows they append lie past the model's own, and the factor, z, V, F and the
// tables of the leading rows do not depend on later rows, so truncating back to the
// model's rows restores it. What the loop overwrites that a truncate does not bring
// back is saved and restored: the resident posterior (both ping-pong buffers and
// their tags: the lattice steps write them), the kept result's validity, the path
// counters (the loop's steps go to the context's planner counters instead), the
// factor's and V's extent (a failed loop returns through the same restore: on any
// error the model is as before the call). A copy
// of A, V and F (~320 MB per model at 128 x 128, N = 2048) and the allocations it
// took cost more than the whole loop (profiles/r06a_choi: ~36 of 44 ms for 8 seeds).
struct PlanSave {
  int64_t NH0 = 0;
  double* res = nullptr;   // device copy of m->res ([2][2][res_M]), or null
  int64_t res_n[2];
  uint64_t res_gen[2], res_tick[2], tick;
  int res_depth[2];
  bool spec_valid, spec_max, pred_since_append;
  bool factored;
  int64_t factor_N, v_n;
  int64_t cnt[N_COUNTERS];   // the path counters
};
// doubles of device room plan_enter needs for m's resident posterior
static size_t plan_res_doubles(const mfgp_model* m) { return m->res ? 4 * (size_t)m->res_M : 0; }
// save what the loop may overwrite; `room` (plan_res_doubles) receives the posterior
static int plan_enter(mfgp_model* m, PlanSave& s, double* room) {
  s.NH0 = m->NH;
  bump_serial(m);   // the loop appends in place: no earlier result's holder may read V meanwhile
  s.res = (m->res && room) ? room : nullptr;
  if (s.res) HIP_TRY(hipMemcpyAsync(s.res, m->res, sizeof(double) * 4 * m->res_M, hipMemcpyDeviceToDevice, m->ctx->stream));
  for (int b = 0; b < 2; ++b) {
    s.res_n[b] = m->res_n[b];
    s.res_gen[b] = m->res_gen[b];
    s.res_tick[b] = m->res_tick[b];
    s.res_depth[b] = m->res_depth[b];
  }
  s.tick = m->tick;
  s.spec_valid = m->spec_valid;
  s.spec_max = m->spec_max;
  s.pred_since_append = m->pred_since_append;
  s.factored = m->factored;
  s.factor_N = m->factor_N;
  s.v_n = m->v_n;
  std::memcpy(s.cnt, m->cnt, sizeof(s.cnt));
  return MFGP_OK;
}
// The loop's deferred status entries of m (the ASYNC batch steps register them): the
// loop read the words itself at every chunk's end, and what it found is its caller's
// to return -- a later mfgp_ctx_synchronize must neither raise it again nor drop the
// factor of the restored model.
static void plan_drop_async(mfgp_model* m) {
  auto& as = m->ctx->async_status;
  as.erase(std::remove_if(as.begin(), as.end(), [m](const mfgp_ctx::AsyncStatus& e) { return e.m == m; }), as.end());
}
// back to the model's own rows and state (also after a failed loop: the error is
// the caller's to return: `failed`); the loop's path counters go to the context's
static int plan_leave(mfgp_model* m, const PlanSave& s, bool failed = false) {
  m->gate_dev = nullptr;
  plan_drop_async(m);
  int64_t* p = m->ctx->plan_stats;
  auto took = [&](PathCounter k) { return m->cnt[k] - s.cnt[k]; };
  p[0] += 1;
  p[1] += took(N_INC_FACTOR);
  p[2] += took(N_VSTREAM);
  p[3] += took(N_LATTICE);
  p[4] += took(N_LATTICE_ARG);
  p[5] += took(N_LATTICE_G2);
  p[6] += took(N_FULL_FACTOR);
  p[7] += took(N_FULL_PREDICT);
  std::memcpy(m->cnt, s.cnt, sizeof(s.cnt));
  m->NH = s.NH0;
  bump_serial(m);
  const int64_t N = m->NL + m->NH;
  // the factor of the model's own rows is the one it entered with (the loop wrote
  // rows past them only, also in a step that failed); V likewise, and what the loop's
  // first predict built of it stays. INVARIANT this relies on: between plan_enter and
  // here nothing drops the factor or V's leading rows for real -- ensure_cap keeps a
  // factored model's factor (its !keep branch needs !factored, and plan_enter runs
  // after update_factor), ensure_v copies the valid rows when only the capacity grew
  // (its drop branch needs another grid or no V, and then s.v_n is 0 already), and the
  // loops fail on "factor lost on growth". A path that could drop either inside the
  // loop must clear s.factored / s.v_n too, or this restore would resurrect them.
  m->factored = s.factored;
  m->factor_N = std::min(s.factor_N, N);
  m->v_n = std::max(std::min(m->v_n, N), std::min(s.v_n, N));
  m->F_n = std::min(m->F_n, N);
  m->vc_n = std::min(m->vc_n, N);
  m->tab_n = std::min(m->tab_n, N);
  m->l21c_N = -1;   // (the compact rows in iscr are the loop's now)
  if (failed) {
    // a failed step left its verdict in the status word: the kept factor is a valid
    // one, and the next loop's first decision reads the word before any append resets it
    static const int ok = INT_MAX;
    HIP_TRY(hipMemcpyAsync(m->status, &ok, sizeof(int), hipMemcpyHostToDevice, m->ctx->stream));
  }
  if (s.res && m->res) {
    HIP_TRY(hipMemcpyAsync(m->res, s.res, sizeof(double) * 4 * m->res_M, hipMemcpyDeviceToDevice, m->ctx->stream));
    for (int b = 0; b < 2; ++b) {
      m->res_n[b] = s.res_n[b];
      m->res_gen[b] = s.res_gen[b];
      m->res_tick[b] = s.res_tick[b];
      m->res_depth[b] = s.res_depth[b];
    }
    m->tick = std::max(m->tick, s.tick);
  } else {
    for (int b = 0; b < 2; ++b)
      if (m->res_n[b] > N) m->res_n[b] = -1;
  }
  // the kept result of the model's last predict: spec_out is not written by the loop
  m->spec_valid = s.spec_valid && factor_current(m);
  m->spec_max = s.spec_max && m->spec_valid;
  m->pred_since_append = s.pred_since_append;
  return MFGP_OK;
}

// compute_sample_points (simulator.py:326-374) as a device loop. Each iteration
// is k_choi_select (argmax cell + its mean -> new hifi row, or stop), a 1-row
// bordered append and a one-pass predict with the fused argmax, all gated by a
// device flag, so chunks of iterations are enqueued without a host round trip;
// the host reads the flag once per chunk and truncates the rows that a stopped
// loop did not append (the leading rows' factor and V stay valid).
int mfgp_sample_points(mfgp_model* model, double threshold, int64_t max_points, double* points, int64_t* count) {
  const Entry entry(model);
  int rc = entry.rc;
  if (rc) return rc;
  if (!count || (max_points > 0 && !points)) return set_err(MFGP_ERR_ARG, "null output");
  if (max_points < 0) return set_err(MFGP_ERR_ARG, "negative max_points");
  if (model->M <= 0) return set_err(MFGP_ERR_ARG, "no grid: call mfgp_set_grid first");
  *count = 0;
  mfgp_ctx* c = model->ctx;
  if (!c->incremental) return set_err(MFGP_ERR_ARG, "mfgp_sample_points needs incremental updates enabled");
  // earlier ASYNC steps' verdicts first: the loop's decisions read the status word
  if (!c->async_status.empty() && (rc = mfgp_ctx_synchronize(c))) return rc;
  if ((rc = update_factor(model))) return rc;
  // the reference works on a deep copy (sim:339); here on the model itself, brought
  // back to its own rows and state at the end (plan_enter / plan_leave)
  mfgp_model* t = model;
  const int64_t M = t->M;
  // workspace: mu, var [M] | vmax | vargmax | state {gate, count} | points [max_points][2] |
  // the saved resident posterior
  const size_t npt = 2 * (size_t)std::max<int64_t>(max_points, 1);
  const size_t nd = 2 * (size_t)M + 4 + npt + plan_res_doubles(t);
  if ((rc = ensure_ws(c, sizeof(double) * nd))) return rc;
  double* mu_s = c->ws;
  double* var_s = mu_s + M;
  double* vmax = var_s + M;
  int64_t* vargmax = reinterpret_cast<int64_t*>(vmax + 1);
  int64_t* state = vargmax + 1;
  double* pts = reinterpret_cast<double*>(state + 2);
  int* gate = reinterpret_cast<int*>(state);
  PlanSave sv;
  if ((rc = plan_enter(t, sv, pts + npt))) return rc;
  auto fail = [&](int code) {
    (void)plan_leave(t, sv, true);
    (void)hipStreamSynchronize(c->stream);   // (the restore copies read ws)
    return code;
  };
  // initial posterior (sim:340-342)
  if ((rc = batch_run(&t, 1, nullptr, nullptr, nullptr, mu_s, var_s, vmax, vargmax, 0, false, true))) return fail(rc);
  const int64_t st0[2] = {1, 0};
  if (hipMemcpyAsync(state, st0, sizeof(st0), hipMemcpyHostToDevice, c->stream) != hipSuccess)
    return fail(set_err(MFGP_ERR_DEVICE, "state upload failed"));
  const int64_t NH0 = t->NH;
  int64_t done = 0;
  bool active = true;
  constexpr int64_t CH = 32;   // iterations per chunk (two descriptors each)
  while (active && done < max_points) {
    const int64_t C = std::min<int64_t>(CH, max_points - done);
    const int64_t N = t->NL + t->NH;
    if ((rc = ensure_cap(t, N + C)) || (rc = ensure_v(t))) return fail(rc);
    if (!factor_current(t)) return fail(set_err(MFGP_ERR_DEVICE, "sample_points: factor lost on growth"));
    int slot;
    GPDesc* hd = acquire_slot(c, slot, rc);
    if (!hd) return fail(rc);
    for (int64_t it = 0; it < C; ++it) {
      t->NH += 1;   // assume the iteration runs; truncated below if the loop stopped
      GPDesc& fd = hd[2 * it];
      if ((rc = fill_inc_desc(fd, t))) return fail(rc);
      fd.mu = mu_s;
      fd.vmax = vmax;
      fd.vargmax = vargmax;
      fd.gate = gate;
      if (c->fused) {   // the iteration's append and predict in one launch
        fd.var = var_s;
        fd.tiles = 1;
      }
      mark_inc_factor(t);
      GPDesc& pd = hd[2 * it + 1];
      fill_desc(pd, t);
      set_vstream_rows(pd, t);
      pd.mu = mu_s;
      pd.var = var_s;
      pd.vmax = vmax;
      pd.vargmax = vargmax;
      pd.gate = gate;
      t->v_n = t->NL + t->NH;
    }
    set_rsplit(c, hd + 1, 1);
    for (int64_t i = 0; i < 2 * C; ++i) hd[i].rsplit = hd[1].rsplit;
    const GPDesc* dd = nullptr;
    if ((rc = upload_slot(c, slot, (int)(2 * C), &dd))) return fail(rc);
    const int vf = t->dtype == MFGP_F32 ? 1 : 0;
    for (int64_t it = 0; it < C; ++it) {
      const bool ok = hipSuccess == launch_choi_select(dd + 2 * it, threshold, pts, max_points, c->stream) &&
                      (c->fused ? hipSuccess == launch_inc_stream(dd + 2 * it, 1,
                                                                   hd[2 * it].nprod + ntiles_wg(M, hd[2 * it].rsplit, vf),
                                                                   vf, c->stream)
                                : (hipSuccess == launch_inc_factor(dd + 2 * it, 1, hd[2 * it].nprod, vf, c->stream) &&
                                   hipSuccess == launch_vstream(dd + 2 * it + 1, 1, ntiles_wg(M, hd[2 * it + 1].rsplit, vf),
                                                                vf, c->stream)));
      if (!ok) return fail(set_err(MFGP_ERR_DEVICE, "sample_points: launch failed"));
    }
    if ((rc = release_slot(c, slot))) return fail(rc);
    int64_t st[2] = {0, 0};
    if (hipMemcpyAsync(st, state, sizeof(st), hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
        hipStreamSynchronize(c->stream) != hipSuccess)
      return fail(set_err(MFGP_ERR_DEVICE, "sample_points: state read failed"));
    active = (int)st[0] != 0;
    const int64_t ran = st[1] - done;
    done = st[1];
    if (ran < C) {
      // the loop stopped inside this chunk: drop the rows it did not append
      if ((rc = mfgp_truncate(t, NH0 + done))) return fail(rc);
    }
    if ((rc = read_status(t))) return fail(rc);
  }
  if (done > 0 && hipMemcpy(points, pts, sizeof(double) * 2 * done, hipMemcpyDefault) != hipSuccess)
    return fail(set_err(MFGP_ERR_DEVICE, "sample_points: copy out failed"));
  *count = done;
  if ((rc = plan_leave(t, sv))) return rc;
  return mfgp_ctx_synchronize(c);   // (the posterior's restore copy: ws is reused by the next call)
}

// compute_sample_points for a batch of models (the Choi planner's sample-set
// selection of many seeds, sim:326-374) stepped together: per iteration ONE
// k_choi_select_batch (every model's decision from its fused max / argmax) and ONE
// batched append + predict of every model's chosen row through the general batch
// step -- the lattice step where the batch takes it (its kernels and the V stream's
// honour each model's device gate, so a model past its threshold skips the rest of
// the chunk) -- with one host synchronisation per CH iterations. Each model works on
// its own rows past its own (sim:339's deep copy: plan_enter / plan_leave bring it
// back); the chosen points are the single-model loop's, up to the rounding of the
// batch step (ties decided by it).
int mfgp_batch_sample_points(mfgp_model** models, int count, const double* thresholds, int64_t max_points,
                             double* points, int64_t* counts) {
  const auto tp0 = std::chrono::steady_clock::now();
  const DeviceGuard dg_((models && count > 0 && models[0]) ? models[0]->ctx->device : -1);
  if (const int rc_ = settle((models && count > 0 && models[0]) ? models[0]->ctx : nullptr)) return rc_;
  if (count <= 0 || !models || !thresholds || !counts || (max_points > 0 && !points))
    return set_err(MFGP_ERR_ARG, "bad batch_sample_points arguments");
  if (max_points < 0) return set_err(MFGP_ERR_ARG, "negative max_points");
  mfgp_ctx* c = models[0]->ctx;
  if (!c->incremental) return set_err(MFGP_ERR_ARG, "mfgp_batch_sample_points needs incremental updates enabled");
  int rc = MFGP_OK;
  for (int b = 0; b < count; ++b) {
    if ((rc = check_model(models[b]))) return rc;
    if (models[b]->ctx != c) return set_err(MFGP_ERR_ARG, "batch models must share one context");
    if (models[b]->dtype != models[0]->dtype) return set_err(MFGP_ERR_ARG, "batch models must share one dtype");
    if (models[b]->M <= 0) return set_err(MFGP_ERR_ARG, "model %d: no grid (call mfgp_set_grid first)", b);
    for (int b2 = 0; b2 < b; ++b2)
      if (models[b2] == models[b]) return set_err(MFGP_ERR_ARG, "model %d appears twice in the batch", b);
    counts[b] = 0;
  }
  // earlier ASYNC steps' verdicts first: the loop's decisions read the status words
  if (!c->async_status.empty() && (rc = mfgp_ctx_synchronize(c))) return rc;
  for (int b = 0; b < count; ++b)
    if ((rc = update_factor(models[b]))) return rc;
  mfgp_model* const* t = models;
  // device state: mu, var [sum M] | vmax [B] | vargmax [B] | state [B][2] | thr [B] | moff [B] |
  // Ms [B] | grids [B] | status words [B] | xn [B][2] | yn [B] | pos [B] | points [B][max_points][2] |
  // the models' saved resident posteriors
  std::vector<int64_t> moff(count), Ms(count);
  int64_t Mtot = 0;
  size_t nres = 0;
  for (int b = 0; b < count; ++b) {
    moff[b] = Mtot;
    Ms[b] = t[b]->M;
    Mtot += t[b]->M;
    nres += plan_res_doubles(t[b]);
  }
  const int64_t P = std::max<int64_t>(max_points, 1);
  // one 8-byte slot per entry (pos's ints take a slot each); the offsets below are
  // the only description of the layout, and the allocation is their end
  const size_t B_ = (size_t)count;
  const size_t o_mu = 0, o_var = o_mu + (size_t)Mtot, o_vmax = o_var + (size_t)Mtot, o_varg = o_vmax + B_;
  const size_t o_state = o_varg + B_, o_thr = o_state + 2 * B_, o_moff = o_thr + B_, o_Ms = o_moff + B_;
  const size_t o_grids = o_Ms + B_, o_stat = o_grids + B_, o_xn = o_stat + B_, o_yn = o_xn + 2 * B_, o_pos = o_yn + B_;
  const size_t o_pts = o_pos + B_, o_res = o_pts + 2 * B_ * (size_t)P, nd = o_res + nres;
  double* ws = nullptr;
  if (hipMalloc(&ws, sizeof(double) * nd) != hipSuccess)
    return set_err(MFGP_ERR_DEVICE, "batch_sample_points: out of memory");
  std::vector<PlanSave> sv(count);
  int entered = 0;
  auto fail = [&](int code) {
    for (int b = 0; b < entered; ++b) (void)plan_leave(t[b], sv[b], true);
    (void)hipStreamSynchronize(c->stream);   // (the restore copies read ws)
    (void)hipFree(ws);
    return code;
  };
  for (size_t b = 0, off = o_res; b < B_; off += plan_res_doubles(t[b]), ++b) {
    if ((rc = plan_enter(t[b], sv[b], ws + off))) return fail(rc);
    ++entered;
  }
  double* mu = ws + o_mu;
  double* var = ws + o_var;
  double* vmax = ws + o_vmax;
  int64_t* vargmax = reinterpret_cast<int64_t*>(ws + o_varg);
  int64_t* state = reinterpret_cast<int64_t*>(ws + o_state);
  double* thr = ws + o_thr;
  int64_t* moff_d = reinterpret_cast<int64_t*>(ws + o_moff);
  int64_t* Ms_d = reinterpret_cast<int64_t*>(ws + o_Ms);
  const double** grids_d = reinterpret_cast<const double**>(ws + o_grids);
  const int** stat_d = reinterpret_cast<const int**>(ws + o_stat);
  double* xn = ws + o_xn;
  double* yn = ws + o_yn;
  int* pos_d = reinterpret_cast<int*>(ws + o_pos);
  double* pts = ws + o_pts;
  std::vector<int64_t> st(2 * count);
  std::vector<const double*> grids(count);
  std::vector<const int*> stat(count);
  for (int b = 0; b < count; ++b) {
    st[2 * b] = 1;
    st[2 * b + 1] = 0;
    grids[b] = t[b]->grid;
    stat[b] = t[b]->status;
  }
  hipStream_t s = c->stream;
  if (hipMemcpyAsync(state, st.data(), sizeof(int64_t) * 2 * count, hipMemcpyHostToDevice, s) != hipSuccess ||
      hipMemcpyAsync(thr, thresholds, sizeof(double) * count, hipMemcpyDefault, s) != hipSuccess ||
      hipMemcpyAsync(moff_d, moff.data(), sizeof(int64_t) * count, hipMemcpyHostToDevice, s) != hipSuccess ||
      hipMemcpyAsync(Ms_d, Ms.data(), sizeof(int64_t) * count, hipMemcpyHostToDevice, s) != hipSuccess ||
      hipMemcpyAsync(grids_d, grids.data(), sizeof(double*) * count, hipMemcpyHostToDevice, s) != hipSuccess ||
      hipMemcpyAsync(stat_d, stat.data(), sizeof(int*) * count, hipMemcpyHostToDevice, s) != hipSuccess)
    return fail(set_err(MFGP_ERR_DEVICE, "batch_sample_points: state upload failed"));
  // the initial posteriors and their max / argmax (sim:340-342)
  if ((rc = batch_run(const_cast<mfgp_model**>(t), count, nullptr, nullptr, nullptr, mu, var, vmax, vargmax, 0,
                      false, true)))
    return fail(rc);
  for (int b = 0; b < count; ++b) t[b]->gate_dev = reinterpret_cast<int*>(state + 2 * b);
  // the models still running (the batch step's members; a stopped one leaves at the
  // next chunk boundary), their offsets into mu / var and indices into vmax
  std::vector<int> live(count);
  for (int b = 0; b < count; ++b) live[b] = b;
  constexpr int64_t CH = 32;
  int64_t it_done = 0;
  const auto tp1 = std::chrono::steady_clock::now();
  while (!live.empty() && it_done < max_points) {
    const int64_t C = std::min<int64_t>(CH, max_points - it_done);
    // the live models are the batch step's members, in batch order: their rows at
    // their member places (pos), their outputs at their own offsets / indices
    std::vector<mfgp_model*> lm;
    std::vector<int64_t> lk, loff;
    std::vector<int> lvi, pos(count, -1);
    for (int b : live) {
      pos[b] = (int)lm.size();
      lm.push_back(t[b]);
      lk.push_back(1);
      loff.push_back(moff[b]);
      lvi.push_back(b);
    }
    if (hipMemcpyAsync(pos_d, pos.data(), sizeof(int) * count, hipMemcpyHostToDevice, s) != hipSuccess)
      return fail(set_err(MFGP_ERR_DEVICE, "batch_sample_points: upload failed"));
    for (int64_t it = 0; it < C; ++it) {
      if (launch_choi_select_batch(count, pos_d, state, stat_d, thr, vmax, vargmax, mu, moff_d, grids_d, Ms_d, xn, yn,
                                   pts, max_points, s) != hipSuccess)
        return fail(set_err(MFGP_ERR_DEVICE, "batch_sample_points: launch failed"));
      if ((int)lm.size() == count)
        rc = batch_run(lm.data(), count, xn, yn, lk.data(), mu, var, vmax, vargmax, MFGP_ASYNC, true, true);
      else
        rc = batch_run(lm.data(), (int)lm.size(), xn, yn, lk.data(), mu, var, vmax, vargmax, MFGP_ASYNC, true, true,
                       loff.data(), lvi.data());
      if (rc) return fail(rc);
    }
    it_done += C;
    if (hipMemcpyAsync(st.data(), state, sizeof(int64_t) * 2 * count, hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess)
      return fail(set_err(MFGP_ERR_DEVICE, "batch_sample_points: state read failed"));
    for (int b : live)
      if ((rc = read_status(t[b]))) return fail(rc);
    std::vector<int> keep;
    for (int b : live)
      if ((int)st[2 * b] != 0) keep.push_back(b);
    live.swap(keep);
  }
  const auto tp2 = std::chrono::steady_clock::now();
  for (int b = 0; b < count; ++b) {
    counts[b] = st[2 * b + 1];
    if (counts[b] > 0 && hipMemcpy(points + 2 * (size_t)b * (size_t)P, pts + 2 * (size_t)b * (size_t)P,
                                   sizeof(double) * 2 * counts[b], hipMemcpyDefault) != hipSuccess)
      return fail(set_err(MFGP_ERR_DEVICE, "batch_sample_points: copy out failed"));
  }
  for (int b = 0; b < count; ++b) (void)plan_leave(t[b], sv[b]);
  entered = 0;
  const bool sync_ok = hipStreamSynchronize(s) == hipSuccess;   // (the restore copies read ws)
  (void)hipFree(ws);
  const auto tp3 = std::chrono::steady_clock::now();
  auto us = [](std::chrono::steady_clock::duration dt) {
    return (int64_t)std::chrono::duration_cast<std::chrono::microseconds>(dt).count();
  };
  c->plan_stats[8] += us(tp1 - tp0);
  c->plan_stats[9] += us(tp2 - tp1);
  c->plan_stats[10] += us(tp3 - tp2);
  return sync_ok ? MFGP_OK : set_err(MFGP_ERR_DEVICE, "batch_sample_points: restore failed");
}

// The greedy integrated-variance planner (mfgp_plan_ivr.hip): n_points cells chosen one
// after another, each the allowed cell whose measurement lowers the weighted posterior
// variance of the whole grid most, given the picks before it. Each iteration is
// k_ivr_pick (argmax of S / (var + sigma_H + jitter), the cell and its posterior mean
// -> the next hifi row, or the gate closed), the general batch step of one model on
// that row (the lattice step where its gates take it, else the fused V stream), then
// the rank-one update of the numerators S from one covariance product over the
// resident V (k_plan_x, k_cov_dot, k_cov_psum, the K** x term, k_cov_apply). S_0 (and
// every `refresh` picks, S again) is k_ivr_partial's numerators over all cells: the
// only GEMM. Chunks of iterations are enqueued behind the device gate with one status
// read per chunk, on the caller's model (plan_enter / plan_leave), as
// mfgp_sample_points; a chunk ends where a refresh is due.
int mfgp_plan_ivr(mfgp_model* model, const double* w, int64_t ldw, const int64_t* cand, int64_t nc,
                  int64_t n_points, double min_gain, int refresh, int64_t* cells, double* points, double* gains,
                  int64_t* count) {
  const Entry entry(model);
  int rc = entry.rc;
  if (rc) return rc;
  mfgp_model* t = model;
  mfgp_ctx* c = t->ctx;
  const int64_t M = t->M;
  if (!count) return set_err(MFGP_ERR_ARG, "mfgp_plan_ivr: null count");
  if (n_points < 0) return set_err(MFGP_ERR_ARG, "mfgp_plan_ivr: negative n_points");
  if (refresh < 0) return set_err(MFGP_ERR_ARG, "mfgp_plan_ivr: negative refresh");
  if (n_points > 0 && (!cells || !points || !gains)) return set_err(MFGP_ERR_ARG, "mfgp_plan_ivr: null output");
  if (t->dtype != MFGP_F64)
    return set_err(MFGP_ERR_ARG, "mfgp_plan_ivr: MFGP_F32 models (fp32 V) are not supported; use an MFGP_F64 model");
  if (M <= 0 || !t->grid) return set_err(MFGP_ERR_ARG, "mfgp_plan_ivr: the model has no grid (mfgp_set_grid)");
  if (!c->incremental) return set_err(MFGP_ERR_ARG, "mfgp_plan_ivr needs incremental updates enabled");
  if (w && ldw < M)
    return set_err(MFGP_ERR_ARG, "mfgp_plan_ivr: ldw = %lld is less than M = %lld", (long long)ldw, (long long)M);
  if (nc < 0) return set_err(MFGP_ERR_ARG, "mfgp_plan_ivr: negative candidate count");
  if (!cand && nc != M)
    return set_err(MFGP_ERR_ARG, "mfgp_plan_ivr: a NULL candidate list means all %lld cells (got nc = %lld)",
                   (long long)M, (long long)nc);
  for (int64_t j = 0; cand && j < nc; ++j)
    if (cand[j] < 0 || cand[j] >= M)
      return set_err(MFGP_ERR_ARG, "mfgp_plan_ivr: cand[%lld] = %lld is outside the grid's cells [0, %lld)",
                     (long long)j, (long long)cand[j], (long long)M);
  const bool w_host = w && !is_device_ptr(w);
  if (w_host && !all_finite(w, M)) return set_err(MFGP_ERR_ARG, "mfgp_plan_ivr: the weights must be finite");
  if (ivr_segments(M) > 65535)
    return set_err(MFGP_ERR_ARG, "mfgp_plan_ivr: grids of at most %lld cells are supported",
                   (long long)65535 * IVR_SEG * PBM);
  *count = 0;
  if (n_points == 0 || nc == 0) return MFGP_OK;
  // earlier ASYNC steps' verdicts first: the loop's decisions read the status word
  if (!c->async_status.empty() && (rc = mfgp_ctx_synchronize(c))) return rc;
  if ((rc = update_factor(t))) return rc;
  if ((rc = ensure_resident_v(t, "mfgp_plan_ivr"))) return rc;
  const int64_t NH0 = t->NH, N0 = t->NL + t->NH;
  if ((rc = ensure_cap(t, N0 + std::min<int64_t>(n_points, 32))) || (rc = ensure_v(t))) return rc;
  // device state (the context's workspace serves the lattice step): mu, var, S, g, x [M] | tau's
  // partials | vmax | vargmax | state {gate, count} | xn [2] | yn | cells, gains [P] | points [P][2] |
  // cand | host weights | k_ivr_partial's partials | the covariance product's scratch | the
  // saved resident posterior
  const int64_t P = n_points, ntau = plan_tau_parts(M), nseg = ivr_segments(M);
  WsLayout lay;
  const size_t o_mu = lay.take(sizeof(double) * M), o_var = lay.take(sizeof(double) * M);
  const size_t o_S = lay.take(sizeof(double) * M), o_g = lay.take(sizeof(double) * M);
  const size_t o_x = lay.take(sizeof(double) * M), o_tau = lay.take(sizeof(double) * ntau);
  const size_t o_misc = lay.take(sizeof(double) * 8);
  const size_t o_cells = lay.take(sizeof(int64_t) * P), o_gains = lay.take(sizeof(double) * P);
  const size_t o_pts = lay.take(sizeof(double) * 2 * P);
  const size_t o_cand = lay.take(cand ? sizeof(int64_t) * nc : 0);
  const size_t o_w = lay.take(w_host ? sizeof(double) * M : 0);
  const size_t o_part = lay.take(sizeof(double) * (size_t)nseg * M);
  const size_t o_work = lay.take(cov_work_bytes(t, N0 + P));
  const size_t o_res = lay.take(sizeof(double) * plan_res_doubles(t));
  char* ws = nullptr;
  if (hipMalloc(&ws, lay.end) != hipSuccess) {
    (void)hipGetLastError();
    return set_err(MFGP_ERR_DEVICE, "mfgp_plan_ivr: out of memory (%zu bytes of scratch)", lay.end);
  }
  auto at = [&](size_t o) { return reinterpret_cast<double*>(ws + o); };
  double *mu_s = at(o_mu), *var_s = at(o_var), *S = at(o_S), *g = at(o_g), *x = at(o_x), *tau = at(o_tau);
  double* vmax = at(o_misc);
  int64_t* vargmax = reinterpret_cast<int64_t*>(vmax + 1);
  int64_t* state = vargmax + 1;
  double *xn = reinterpret_cast<double*>(state + 2), *yn = xn + 2;
  int* gate = reinterpret_cast<int*>(state);
  int64_t* dcells = reinterpret_cast<int64_t*>(ws + o_cells);
  int64_t* dcand = cand ? reinterpret_cast<int64_t*>(ws + o_cand) : nullptr;
  hipStream_t s = c->stream;
  PlanSave sv;
  bool entered = false;
  auto fail = [&](int code) {
    if (entered) (void)plan_leave(t, sv, true);
    (void)hipStreamSynchronize(s);   // (the restore copies read ws)
    (void)hipFree(ws);
    return code;
  };
  if ((rc = plan_enter(t, sv, at(o_res)))) return fail(rc);
  entered = true;
  const double* dw = w;
  if (w_host) {
    if (hipMemcpyAsync(at(o_w), w, sizeof(double) * M, hipMemcpyHostToDevice, s) != hipSuccess)
      return fail(set_err(MFGP_ERR_DEVICE, "mfgp_plan_ivr: upload failed"));
    dw = at(o_w);
  }
  const int64_t st0[2] = {1, 0};
  if ((cand && hipMemcpyAsync(dcand, cand, sizeof(int64_t) * nc, hipMemcpyHostToDevice, s) != hipSuccess) ||
      hipMemcpyAsync(state, st0, sizeof(st0), hipMemcpyHostToDevice, s) != hipSuccess)
    return fail(set_err(MFGP_ERR_DEVICE, "mfgp_plan_ivr: upload failed"));
  // the initial posterior, and S_0
  if ((rc = batch_run(&t, 1, nullptr, nullptr, nullptr, mu_s, var_s, vmax, vargmax, MFGP_ASYNC, false, true)))
    return fail(rc);
  auto numerators = [&]() -> int {
    GPDesc d;
    fill_desc(d, t);
    HIP_TRY(launch_ivr_partial(d, nullptr, M, dw, 1, M, at(o_part), s));
    HIP_TRY(launch_plan_ssum(at(o_part), (int)nseg, M, S, s));
    return MFGP_OK;
  };
  if ((rc = numerators())) return fail(rc);
  CovWork cw;
  if ((rc = cov_work_init(t, ws + o_work, N0 + P, cw))) return fail(rc);
  cw.a.x = x;
  cw.a.S = S;
  cw.a.g = g;
  cw.a.tau_part = tau;
  cw.a.ntau = (int)ntau;
  cw.a.gate = gate;
  PlanPick q{};
  q.S = S;
  q.var = var_s;
  q.mu = mu_s;
  q.grid = t->grid;
  q.cand = dcand;
  q.nc = nc;
  q.noise = cw.a.h.noiseH;
  q.jitter = cw.a.h.jitter;
  q.min_gain = min_gain;
  q.n_points = n_points;
  q.state = state;
  q.status = t->status;
  q.xn = xn;
  q.yn = yn;
  q.cells = dcells;
  q.gains = at(o_gains);
  q.pts = at(o_pts);
  t->gate_dev = gate;
  int64_t done = 0;
  bool active = true;
  constexpr int64_t CH = 32;   // iterations per chunk
  const int64_t one = 1;
  while (active && done < n_points) {
    int64_t C = std::min<int64_t>(CH, n_points - done);
    if (refresh > 0) C = std::min<int64_t>(C, refresh - done % refresh);
    const int64_t N = t->NL + t->NH;
    if ((rc = ensure_cap(t, N + C)) || (rc = ensure_v(t))) return fail(rc);
    if (!factor_current(t)) return fail(set_err(MFGP_ERR_DEVICE, "mfgp_plan_ivr: factor lost on growth"));
    q.status = t->status;
    if (refresh > 0 && done > 0 && done % refresh == 0 && (rc = numerators())) return fail(rc);
    for (int64_t it = 0; it < C; ++it) {
      if (launch_ivr_pick(q, s) != hipSuccess) return fail(set_err(MFGP_ERR_DEVICE, "mfgp_plan_ivr: launch failed"));
      if ((rc = batch_run(&t, 1, xn, yn, &one, mu_s, var_s, vmax, vargmax, MFGP_ASYNC, true, true))) return fail(rc);
      if (done + it + 1 >= n_points) break;   // the last pick: no score is read after it
      const int64_t row = t->NL + t->NH - 1;
      if (launch_plan_x(static_cast<const double*>(t->V), t->vld, row, M, dw, g, x, tau, gate, s) != hipSuccess)
        return fail(set_err(MFGP_ERR_DEVICE, "mfgp_plan_ivr: launch failed"));
      if ((rc = cov_work_run(t, cw, row + 1))) return fail(rc);
    }
    int64_t st[2] = {0, 0};
    if (hipMemcpyAsync(st, state, sizeof(st), hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess)
      return fail(set_err(MFGP_ERR_DEVICE, "mfgp_plan_ivr: state read failed"));
    active = (int)st[0] != 0;
    const int64_t ran = st[1] - done;
    done = st[1];
    if (ran < C) {
      // the loop stopped inside this chunk: drop the rows it did not append
      if ((rc = mfgp_truncate(t, NH0 + done))) return fail(rc);
    }
    if ((rc = read_status(t))) return fail(rc);
  }
  if (done > 0 && (hipMemcpy(cells, dcells, sizeof(int64_t) * done, hipMemcpyDeviceToHost) != hipSuccess ||
                   hipMemcpy(gains, q.gains, sizeof(double) * done, hipMemcpyDeviceToHost) != hipSuccess ||
                   hipMemcpy(points, q.pts, sizeof(double) * 2 * done, hipMemcpyDefault) != hipSuccess))
    return fail(set_err(MFGP_ERR_DEVICE, "mfgp_plan_ivr: copy out failed"));
  *count = done;
  (void)plan_leave(t, sv);
  const bool sync_ok = mfgp_ctx_synchronize(c) == MFGP_OK;   // (the posterior's restore copy reads ws)
  (void)hipFree(ws);
  return sync_ok ? MFGP_OK : set_err(MFGP_ERR_DEVICE, "mfgp_plan_ivr: restore failed");
}

// Voronoi-cell reductions (simulator.py:194-323) on the device. Inputs may be
// host or device memory (host ones are staged through the context workspace);
// outputs likewise. Synchronous. field (host, [ncells]) or null: cell i reads
// w / var of seed field[i] ([nfield][M] each; the lockstep simulations' batch).
static int cell_reduce_impl(mfgp_ctx* c, const double* grid, int64_t M, int ncells, const int* vstart,
                            const double* verts, const double* seeds, const int* field, int nfield, const double* w,
                            const double* f, const double* var, double* out, int64_t* argmax) {
  if (!c) return set_err(MFGP_ERR_ARG, "null ctx");
  if (M < 0 || ncells < 0 || (M > 0 && !grid) || (ncells > 0 && (!vstart || !verts || !seeds || !out || !argmax)))
    return set_err(MFGP_ERR_ARG, "bad cell_reduce arguments");
  if (field && nfield < 1) return set_err(MFGP_ERR_ARG, "nfield must be >= 1");
  if (M == 0 || ncells == 0) {
    for (int i = 0; i < ncells; ++i) {
      for (int j = 0; j < 6; ++j) out[6 * i + j] = (j == 5) ? -HUGE_VAL : 0.0;
      argmax[i] = -1;
    }
    return MFGP_OK;
  }
  // vertex counts (the offsets must be readable on the host)
  if (is_device_ptr(vstart)) return set_err(MFGP_ERR_ARG, "vstart must be host memory");
  if (field && is_device_ptr(field)) return set_err(MFGP_ERR_ARG, "field must be host memory");
  if (vstart[0] != 0) return set_err(MFGP_ERR_ARG, "vstart[0] must be 0");
  for (int i = 0; i < ncells; ++i) {
    if (vstart[i + 1] - vstart[i] > 256 || vstart[i + 1] < vstart[i])
      return set_err(MFGP_ERR_ARG, "cell %d: bad vertex count", i);
    if (field && (field[i] < 0 || field[i] >= nfield)) return set_err(MFGP_ERR_ARG, "cell %d: field out of range", i);
  }
  const int64_t nf = field ? nfield : 1;
  const int64_t nv = vstart[ncells];
  const int64_t npart = cell_partial_doubles(M, ncells);
  // workspace layout (doubles): grid 2M | w nf M | f M | var nf M | verts 2nv | seeds 2n | part | out 6n |
  // argmax n | vstart | field; an input already in device memory is read in place and
  // takes no room (the lockstep driver's w / var at configs[4] scale had
  // kept ~32 MB of workspace that was never written)
  auto host_n = [](const double* p, int64_t n) -> int64_t { return (p && !is_device_ptr(p)) ? n : 0; };
  const int64_t off_g = 0, off_w = off_g + host_n(grid, 2 * M), off_f = off_w + host_n(w, nf * M);
  const int64_t off_v = off_f + host_n(f, M), off_vx = off_v + host_n(var, nf * M);
  const int64_t off_s = off_vx + 2 * nv, off_p = off_s + 2 * ncells, off_o = off_p + npart;
  const int64_t off_a = off_o + 6 * ncells, off_i = off_a + ncells, off_fd = off_i + (ncells + 2) / 2 + 1;
  const int64_t total = off_fd + (ncells + 1) / 2 + 1;
  int rc = ensure_ws(c, sizeof(double) * total);
  if (rc) return rc;
  double* ws = c->ws;
  hipStream_t s = c->stream;
  auto stage = [&](const double* p, int64_t n, int64_t off) -> const double* {
    if (!p) return nullptr;
    if (is_device_ptr(p)) return p;
    if (hipMemcpyAsync(ws + off, p, sizeof(double) * n, hipMemcpyHostToDevice, s) != hipSuccess) return nullptr;
    return ws + off;
  };
  const double* dg = stage(grid, 2 * M, off_g);
  const double* dw = stage(w, nf * M, off_w);
  const double* df = stage(f, M, off_f);
  const double* dv = stage(var, nf * M, off_v);
  const double* dx = stage(verts, 2 * nv, off_vx);
  const double* ds = stage(seeds, 2 * ncells, off_s);
  if (!dg || !dx || !ds || (w && !dw) || (f && !df) || (var && !dv))
    return set_err(MFGP_ERR_DEVICE, "cell_reduce: staging failed");
  int* dvs = reinterpret_cast<int*>(ws + off_i);
  HIP_TRY(hipMemcpyAsync(dvs, vstart, sizeof(int) * (ncells + 1), hipMemcpyHostToDevice, s));
  int* dfd = nullptr;
  if (field) {
    dfd = reinterpret_cast<int*>(ws + off_fd);
    HIP_TRY(hipMemcpyAsync(dfd, field, sizeof(int) * ncells, hipMemcpyHostToDevice, s));
  }
  const bool dev_out = is_device_ptr(out) && is_device_ptr(argmax);
  double* o = dev_out ? out : ws + off_o;
  int64_t* a = dev_out ? argmax : reinterpret_cast<int64_t*>(ws + off_a);
  HIP_TRY(launch_cell_reduce(dg, M, dx, dvs, ncells, ds, dw, df, dv, dfd, ws + off_p, o, a, s));
  if (!dev_out) {
    HIP_TRY(hipMemcpyAsync(out, o, sizeof(double) * 6 * ncells, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(argmax, a, sizeof(int64_t) * ncells, hipMemcpyDeviceToHost, s));
  }
  HIP_TRY(hipStreamSynchronize(s));
  return MFGP_OK;
}

int mfgp_cell_reduce(mfgp_ctx* c, const double* grid, int64_t M, int ncells, const int* vstart, const double* verts,
                     const double* seeds, const double* w, const double* f, const double* var, double* out,
                     int64_t* argmax) {
  const DeviceGuard dg_(c ? c->device : -1);
  if (const int rc_ = settle(c)) return rc_;
  return cell_reduce_impl(c, grid, M, ncells, vstart, verts, seeds, nullptr, 1, w, f, var, out, argmax);
}

int mfgp_batch_cell_reduce(mfgp_ctx* c, const double* grid, int64_t M, int ncells, const int* vstart,
                           const double* verts, const double* seeds, const int* field, int nfield, const double* w,
                           const double* f, const double* var, double* out, int64_t* argmax) {
  const DeviceGuard dg_(c ? c->device : -1);
  if (const int rc_ = settle(c)) return rc_;
  if (!field) return set_err(MFGP_ERR_ARG, "null field");
  return cell_reduce_impl(c, grid, M, ncells, vstart, verts, seeds, field, nfield, w, f, var, out, argmax);
}

}  // extern "C"
