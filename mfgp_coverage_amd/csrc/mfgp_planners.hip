// The planners of libmfgp_hip.so: the loops that run on the caller's models in
// place -- the sample-point loops (mfgp_sample_points, mfgp_batch_sample_points) and the
// greedy integrated-variance planner (plan_ivr_run: one loop with two entry points,
// mfgp_batch_plan_ivr and, as its batch of one, mfgp_plan_ivr), all over the batch step
// and on one scaffold (PlanRun: enter, grow, chunk_end, finish, and fail on every error
// path) -- and the host side of the Voronoi-cell reductions (mfgp_cells.hip).
#include <chrono>
#include <cmath>
#include <cstring>

#include "mfgp_host.h"

using namespace mfgp;
using namespace mfgp_host;

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
  mfgp_state::ModelState st;   // what the buffers held (restore_from takes the factor's, V's and the posterior's part)
  bool spec_valid, spec_max, pred_since_append;
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
  s.st = m->st;
  s.spec_valid = m->spec_valid;
  s.spec_max = m->spec_max;
  s.pred_since_append = m->pred_since_append;
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
  // the factor and V of the model's own rows are the ones it entered with, the posterior
  // buffers too where they were saved (ModelState::restore_from, with its invariant: kept
  // today because ensure_cap keeps a factored model's factor, ensure_v moves V's valid rows
  // when only the capacity grew, and the loops fail on "factor lost on growth")
  const bool posterior = s.res && m->res;
  const bool kept = m->st.restore_from(s.st, m->NL + m->NH, posterior);
  if (failed) {
    // a failed step left its verdict in the status word: the kept factor is a valid
    // one, and the next loop's first decision reads the word before any append resets it
    static const int ok = INT_MAX;
    HIP_TRY(hipMemcpyAsync(m->status, &ok, sizeof(int), hipMemcpyHostToDevice, m->ctx->stream));
  }
  if (posterior && kept)
    HIP_TRY(hipMemcpyAsync(m->res, s.res, sizeof(double) * 4 * m->res_M, hipMemcpyDeviceToDevice, m->ctx->stream));
  // the kept result of the model's last predict: spec_out is not written by the loop
  m->spec_valid = s.spec_valid && factor_current(m);
  m->spec_max = s.spec_max && m->spec_valid;
  m->pred_since_append = s.pred_since_append;
  if (!kept)
    return set_err(MFGP_ERR_DEVICE, "planner restore: the factor or V's leading rows were dropped inside the loop "
                                    "(the invariant of ModelState::restore_from); the model is cut to its rows");
  return MFGP_OK;
}

// Before a loop: earlier ASYNC steps' verdicts first (the loop's decisions read the
// status words), then every model's factor.
static int plan_ready(mfgp_ctx* c, mfgp_model* const* t, int count) {
  int rc;
  if (!c->async_status.empty() && (rc = mfgp_ctx_synchronize(c))) return rc;
  for (int b = 0; b < count; ++b)
    if ((rc = update_factor(t[b]))) return rc;
  return MFGP_OK;
}

// What the loops share: the models a loop runs on in place, what plan_enter saved
// of each, the loop's device scratch and its state words, and the steps every loop takes
// the same way. An entry point checks its arguments, lays the scratch out (WsLayout),
// enqueues its iterations in chunks of PLAN_CHUNK behind the device gates and copies its
// results out; from `enter` on, every error returns through `fail`, which leaves the
// models as they were before the call.
constexpr int64_t PLAN_CHUNK = 32;   // iterations enqueued per host synchronisation
struct __attribute__((visibility("hidden"))) PlanRun {   // (its members: no symbols of the library)
  const char* who;            // the entry point, for the messages
  mfgp_ctx* c;
  mfgp_model* const* t;       // the models
  int count;
  std::vector<PlanSave> sv;
  int entered = 0;            // the models plan_enter has saved
  char* ws = nullptr;         // the scratch: the run's own (`mine`, freed with the run) or the context's workspace
  Dev<char> mine;
  int64_t* state = nullptr;   // device [count][2]: {gate, rows appended}
  std::vector<int64_t> st;    // its host image: {1, 0} each for `open`, then as of the last chunk_end
  std::vector<int> live;      // the models whose status chunk_end reads (the batched loop prunes it)
  int64_t done = 0;           // a single-model loop: the rows appended so far

  PlanRun(const char* who_, mfgp_ctx* c_, mfgp_model* const* t_, int n)
      : who(who_), c(c_), t(t_), count(n), sv(n), st(2 * (size_t)n, 0), live(n) {
    for (int b = 0; b < n; ++b) {
      st[2 * b] = 1;
      live[b] = b;
    }
  }
  template <class T = double>
  T* at(size_t o) const {
    return reinterpret_cast<T*>(ws + o);
  }
  bool own(size_t bytes) {
    ws = dev_alloc(mine, c->stream, bytes, A_NO_DRAIN) == MFGP_OK ? mine.get() : nullptr;
    return ws != nullptr;
  }
  // plan_enter for each model; `room`: the models' plan_res_doubles, one after another
  int enter(double* room) {
    for (; entered < count; room += plan_res_doubles(t[entered]), ++entered)
      if (const int rc = plan_enter(t[entered], sv[entered], room)) return rc;
    return MFGP_OK;
  }
  // an error after enter: the models restored, the scratch released; returns code
  int fail(int code) {
    for (int b = 0; b < entered; ++b) (void)plan_leave(t[b], sv[b], true);
    (void)hipStreamSynchronize(c->stream);   // (the restore copies read ws)
    mine.reset();
    return code;
  }
  // the gates opened, the counts zeroed
  hipError_t open() {
    return hipMemcpyAsync(state, st.data(), sizeof(int64_t) * st.size(), hipMemcpyHostToDevice, c->stream);
  }
  // room for C more rows of m, with its factor and V kept
  int grow(mfgp_model* m, int64_t C) {
    int rc;
    if ((rc = ensure_cap(m, m->NL + m->NH + C)) || (rc = ensure_v(m))) return rc;
    if (!factor_current(m)) return set_err(MFGP_ERR_DEVICE, "%s: factor lost on growth", who);
    return MFGP_OK;
  }
  // A chunk's end: the state words read back and the stream drained, then the live
  // models' status words. C >= 0, a single-model loop's chunk of C iterations: `done`
  // follows, and if the loop stopped inside the chunk, the rows it did not append go.
  int chunk_end(int64_t C = -1) {
    int rc;
    if (hipMemcpyAsync(st.data(), state, sizeof(int64_t) * st.size(), hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
        hipStreamSynchronize(c->stream) != hipSuccess)
      return set_err(MFGP_ERR_DEVICE, "%s: state read failed", who);
    if (C >= 0) {
      const int64_t ran = st[1] - done;
      done = st[1];
      if (ran < C && (rc = mfgp_truncate(t[0], sv[0].NH0 + done))) return rc;
    }
    for (int b : live)
      if ((rc = read_status(t[b]))) return rc;
    return MFGP_OK;
  }
  // The loop's end: the models back to their own rows and state, the last wait (the
  // restore copies read ws: the context's, with its deferred verdicts, or the stream's
  // alone), the scratch released. Returns the first failure of the restores and the wait.
  int finish(bool ctx_sync) {
    int rc = MFGP_OK;
    for (int b = 0; b < entered; ++b)
      if (const int r = plan_leave(t[b], sv[b]); r && !rc) rc = r;
    entered = 0;
    const int sync = ctx_sync ? mfgp_ctx_synchronize(c)
                              : (hipStreamSynchronize(c->stream) == hipSuccess ? MFGP_OK : MFGP_ERR_DEVICE);
    mine.reset();
    return rc ? rc : sync;
  }
};

// The greedy integrated-variance planner (mfgp_plan_ivr.hip) behind both of its entry
// points: for each model of a batch stepped together, n_points cells chosen one after
// another, each the allowed cell whose measurement lowers the weighted posterior variance
// of the model's whole grid most, given the picks before it, with per-group quotas on the
// picks. mfgp_plan_ivr is the batch of one (`single`: its own texts and order where its
// checks differ, and its nc counts with a NULL list too). Per iteration: ONE
// k_ivr_pick_batch (every live member's masked argmax of S / (var + sigma_H + jitter), the
// cell and its posterior mean as its next hifi row at its place in xn / yn, or its gate
// closed), ONE batch step of one row each (as mfgp_batch_sample_points calls it: the
// lattice step where its gates take it, else the fused V stream) and, for the rank-one
// update of the numerators S from one covariance product over the resident V, ONE launch
// each of k_plan_x_batch, k_cov_dot_batch, k_cov_psum_batch, k_kss_t_batch, k_kss_out_batch
// and k_cov_apply_batch, which read each member's arguments from a device array uploaded
// once per chunk (the row count of an iteration is the member's own plus the iteration's
// index). S_0, and S again every `refresh` picks, is k_ivr_partial per member over its
// candidate list -- the only GEMM -- scattered into S at the candidates' cells: no other
// cell of S is read. Chunks of iterations are enqueued behind the device gates with one
// status read per chunk, on the caller's models (plan_enter / plan_leave); a chunk ends
// where a refresh is due. A member that stopped leaves the batch at the next chunk
// boundary; its kernels are no-ops behind its gate meanwhile.
static int plan_ivr_run(const char* who, bool single, mfgp_model* const* t, int count, const double* w, int64_t ldw,
                        const int64_t* cand, const int64_t* cand_off, const int32_t* group, const int64_t* quota,
                        int ngroups, int64_t n_points, double min_gain, int refresh, int64_t* cells, int64_t* pos,
                        double* points, double* gains, int64_t* counts) {
  if (n_points < 0) return set_err(MFGP_ERR_ARG, "%s: negative n_points", who);
  if (refresh < 0) return set_err(MFGP_ERR_ARG, "%s: negative refresh", who);
  if (n_points > 0 && (!cells || !points || !gains)) return set_err(MFGP_ERR_ARG, "%s: null output", who);
  int rc = MFGP_OK;
  for (int b = 0; b < count; ++b)
    if ((rc = check_model(t[b]))) return rc;
  mfgp_ctx* c = t[0]->ctx;
  auto too_large = [&](int b) {
    return ivr_segments(t[b]->M) > 65535 ? set_err(MFGP_ERR_ARG, "%s: grids of at most %lld cells are supported", who,
                                                   (long long)65535 * IVR_SEG * PBM)
                                         : MFGP_OK;
  };
  // the members' cells and lists: offsets into the grid-sized arrays (moff) and into cand / group (coff)
  std::vector<int64_t> moff(count), coff(count), ncs(count);
  int64_t Mtot = 0, maxM = 0, ctot = 0;
  for (int b = 0; b < count; ++b) {
    if (t[b]->ctx != c) return set_err(MFGP_ERR_ARG, "%s: batch models must share one context", who);
    for (int b2 = 0; b2 < b; ++b2)
      if (t[b2] == t[b]) return set_err(MFGP_ERR_ARG, "%s: model %d appears twice in the batch", who, b);
    if ((rc = need_f64_grid(t[b], who))) return rc;
    if (!single && (rc = too_large(b))) return rc;
    moff[b] = Mtot;
    Mtot += t[b]->M;
    maxM = std::max(maxM, t[b]->M);
  }
  if (!c->incremental) return set_err(MFGP_ERR_ARG, "%s needs incremental updates enabled", who);
  if (w && ldw < maxM)
    return set_err(MFGP_ERR_ARG, "%s: ldw = %lld is less than %s = %lld", who, (long long)ldw,
                   single ? "M" : "the largest M", (long long)maxM);
  const bool listed = cand || single;   // the counts are cand_off's (the single call's nc: M with a NULL list)
  if (single && cand_off[1] < 0) return set_err(MFGP_ERR_ARG, "%s: negative candidate count", who);
  if (cand && !cand_off) return set_err(MFGP_ERR_ARG, "%s: cand needs cand_off", who);
  if (cand && cand_off[0] != 0) return set_err(MFGP_ERR_ARG, "%s: cand_off[0] must be 0", who);
  for (int b = 0; b < count; ++b) {
    if (listed && cand_off[b + 1] < cand_off[b])
      return set_err(MFGP_ERR_ARG, "%s: cand_off must not decrease (cand_off[%d] = %lld after %lld)", who, b + 1,
                     (long long)cand_off[b + 1], (long long)cand_off[b]);
    coff[b] = listed ? cand_off[b] : ctot;
    ncs[b] = listed ? cand_off[b + 1] - cand_off[b] : t[b]->M;
    ctot = coff[b] + ncs[b];
    if (listed && (rc = check_cells(who, "cand", cand ? cand + coff[b] : nullptr, ncs[b], t[b]->M))) return rc;
  }
  if (quota && !group) return set_err(MFGP_ERR_ARG, "%s: quota needs group", who);
  if (group) {
    if (ngroups < 1 || ngroups > MFGP_PLAN_MAXGROUPS)
      return set_err(MFGP_ERR_ARG, "%s: ngroups = %d is outside [1, %d]", who, ngroups, MFGP_PLAN_MAXGROUPS);
    for (int64_t j = 0; j < ctot; ++j)
      if (group[j] < 0 || group[j] >= ngroups)
        return set_err(MFGP_ERR_ARG, "%s: group[%lld] = %d is outside [0, %d)", who, (long long)j, (int)group[j],
                       ngroups);
    for (int g = 0; quota && g < ngroups; ++g)
      if (quota[g] < 0) return set_err(MFGP_ERR_ARG, "%s: quota[%d] is negative", who, g);
  }
  const bool w_host = w && !is_device_ptr(w);
  for (int b = 0; w_host && b < count; ++b)
    if (finite_rows(w + (int64_t)b * ldw, 1, ldw, t[b]->M) >= 0)
      return single ? set_err(MFGP_ERR_ARG, "%s: the weights must be finite", who)
                    : set_err(MFGP_ERR_ARG, "%s: the weights must be finite (member %d)", who, b);
  if (single && (rc = too_large(0))) return rc;
  for (int b = 0; b < count; ++b) counts[b] = 0;
  if (n_points == 0 || (single && ncs[0] == 0)) return MFGP_OK;
  if ((rc = plan_ready(c, t, count))) return rc;
  std::vector<int64_t> N0(count);
  for (int b = 0; b < count; ++b) {
    if ((rc = ensure_resident_v(t[b], who))) return rc;
    N0[b] = t[b]->NL + t[b]->NH;
    if ((rc = ensure_cap(t[b], N0[b] + std::min<int64_t>(n_points, PLAN_CHUNK))) || (rc = ensure_v(t[b]))) return rc;
  }
  // device state: mu, var, S, g, x [sum M] | tau's partials | vmax, vargmax [B] | state [B][2] | xn [B][2] |
  // yn [B] | cells, pos, gains [B][P] | points [B][P][2] | cand | group | quota | the group counters
  // [B][groups] | host weights [B][max M] | the members' descriptors | k_ivr_partial's partials (the
  // largest member's: the members' GEMMs follow one another) | each member's covariance-product
  // scratch | the saved resident posteriors
  const size_t P = (size_t)n_points, B = (size_t)count, dM = sizeof(double) * (size_t)Mtot;
  const size_t NG = group ? (size_t)ngroups : 0;
  std::vector<int64_t> toff(count);
  std::vector<size_t> o_work(count);
  int64_t ntau_tot = 0;
  size_t part_max = 0, nres = 0;
  for (int b = 0; b < count; ++b) {
    toff[b] = ntau_tot;
    ntau_tot += plan_tau_parts(t[b]->M);
    part_max = std::max(part_max, (size_t)ivr_segments(t[b]->M) * (size_t)ncs[b]);
    nres += plan_res_doubles(t[b]);
  }
  WsLayout lay;
  const size_t o_mu = lay.take(dM), o_var = lay.take(dM), o_S = lay.take(dM), o_g = lay.take(dM), o_x = lay.take(dM);
  const size_t o_tau = lay.take(sizeof(double) * ntau_tot);
  const size_t o_vmax = lay.take(8 * B), o_varg = lay.take(8 * B), o_state = lay.take(16 * B);
  const size_t o_xn = lay.take(16 * B), o_yn = lay.take(8 * B);
  const size_t o_cells = lay.take(8 * B * P), o_pos = lay.take(8 * B * P), o_gains = lay.take(8 * B * P);
  const size_t o_pts = lay.take(16 * B * P);
  const size_t o_cand = lay.take(cand ? sizeof(int64_t) * ctot : 0);
  const size_t o_group = lay.take(group ? sizeof(int32_t) * ctot : 0);
  const size_t o_quota = lay.take(8 * NG), o_gcnt = lay.take(8 * B * NG);
  const size_t o_w = lay.take(w_host ? sizeof(double) * B * maxM : 0);
  const size_t o_desc = lay.take(sizeof(PlanMember) * B);
  const size_t o_part = lay.take(sizeof(double) * part_max);
  for (int b = 0; b < count; ++b) o_work[b] = lay.take(cov_work_bytes(t[b], N0[b] + n_points));
  const size_t o_res = lay.take(sizeof(double) * nres);
  PlanRun run(who, c, t, count);
  if (!run.own(lay.end)) return set_err(MFGP_ERR_DEVICE, "%s: out of memory (%zu bytes of scratch)", who, lay.end);
  double *mu = run.at(o_mu), *var = run.at(o_var), *S = run.at(o_S), *g = run.at(o_g), *x = run.at(o_x);
  double *tau = run.at(o_tau), *vmax = run.at(o_vmax), *xn = run.at(o_xn), *yn = run.at(o_yn);
  int64_t *vargmax = run.at<int64_t>(o_varg), *state = run.state = run.at<int64_t>(o_state);
  int64_t *dcells = run.at<int64_t>(o_cells), *dpos = run.at<int64_t>(o_pos);
  double *dgains = run.at(o_gains), *dpts = run.at(o_pts);
  const int64_t* dcand = cand ? run.at<int64_t>(o_cand) : nullptr;
  const int32_t* dgroup = group ? run.at<int32_t>(o_group) : nullptr;
  const int64_t* dquota = (group && quota) ? run.at<int64_t>(o_quota) : nullptr;
  int64_t* dgcnt = group ? run.at<int64_t>(o_gcnt) : nullptr;
  PlanMember* dm = run.at<PlanMember>(o_desc);
  hipStream_t s = c->stream;
  if ((rc = run.enter(run.at(o_res)))) return run.fail(rc);
  const StagedIn sw(w, count, maxM, ldw, w_host, run.at(o_w));
  auto weights_of = [&](int b) -> const double* { return sw.dev ? sw.dev + (int64_t)b * sw.ld : nullptr; };
  if (sw.upload(s) != hipSuccess ||
      (cand && hipMemcpyAsync(run.at(o_cand), cand, sizeof(int64_t) * ctot, hipMemcpyHostToDevice, s) != hipSuccess) ||
      (group && hipMemcpyAsync(run.at(o_group), group, sizeof(int32_t) * ctot, hipMemcpyHostToDevice, s) != hipSuccess) ||
      (dquota && hipMemcpyAsync(run.at(o_quota), quota, 8 * NG, hipMemcpyHostToDevice, s) != hipSuccess) ||
      (group && hipMemsetAsync(dgcnt, 0, 8 * B * NG, s) != hipSuccess) ||
      hipMemsetAsync(S, 0, dM, s) != hipSuccess || run.open() != hipSuccess)
    return run.fail(set_err(MFGP_ERR_DEVICE, "%s: upload failed", who));
  // the initial posteriors, and every member's S_0
  if ((rc = batch_run(const_cast<mfgp_model**>(t), count, nullptr, nullptr, nullptr, mu, var, vmax, vargmax, MFGP_ASYNC,
                      false, true)))
    return run.fail(rc);
  auto numerators = [&](int b) -> int {
    GPDesc d;
    fill_desc(d, t[b]);
    const int64_t* cb = dcand ? dcand + coff[b] : nullptr;
    HIP_TRY(launch_ivr_partial(d, cb, ncs[b], weights_of(b), 1, t[b]->M, run.at(o_part), s));
    HIP_TRY(launch_plan_scatter(run.at(o_part), (int)ivr_segments(t[b]->M), ncs[b], cb, S + moff[b], s));
    return MFGP_OK;
  };
  std::vector<CovWork> cw(count);
  bool any_sep = false;
  for (int b = 0; b < count; ++b) {
    if ((rc = numerators(b)) || (rc = cov_work_init(t[b], run.ws + o_work[b], N0[b] + n_points, cw[b])))
      return run.fail(rc);
    any_sep = any_sep || cw[b].sep;
    t[b]->gate_dev = reinterpret_cast<int*>(state + 2 * b);
  }
  // member b's arguments as of this chunk (V, its leading dimension and the status word may move
  // when the capacity grows), with its row at place `place` of xn / yn
  auto describe = [&](int b, int place) {
    PlanMember m{};
    m.a = cw[b].a;
    m.a.V = static_cast<const double*>(t[b]->V.get());
    m.a.vld = t[b]->vld;
    m.a.N = N0[b];
    m.a.x = x + moff[b];
    m.a.S = S + moff[b];
    m.a.g = g + moff[b];
    m.a.tau_part = tau + toff[b];
    m.a.ntau = (int)plan_tau_parts(t[b]->M);
    m.a.gate = reinterpret_cast<int*>(state + 2 * b);
    m.sep = cw[b].sep ? 1 : 0;
    m.a.kx = m.sep ? cw[b].kx : nullptr;
    m.k = cw[b].k;
    m.T = cw[b].T;
    m.kxo = cw[b].kx;
    m.nseg = (int)cov_segments(t[b]->M);
    m.w = weights_of(b);
    PlanPick& q = m.q;
    q.S = m.a.S;
    q.var = var + moff[b];
    q.mu = mu + moff[b];
    q.grid = t[b]->grid;
    q.cand = dcand ? dcand + coff[b] : nullptr;
    q.nc = ncs[b];
    q.noise = m.a.h.noiseH;
    q.jitter = m.a.h.jitter;
    q.min_gain = min_gain;
    q.n_points = n_points;
    q.state = state + 2 * b;
    q.status = t[b]->status;
    q.xn = xn + 2 * place;
    q.yn = yn + place;
    q.cells = dcells + (size_t)b * P;
    q.gains = dgains + (size_t)b * P;
    q.pts = dpts + 2 * (size_t)b * P;
    q.pos = dpos + (size_t)b * P;
    q.group = dgroup ? dgroup + coff[b] : nullptr;
    q.quota = dquota;
    q.gcount = dgcnt ? dgcnt + (size_t)b * NG : nullptr;
    return m;
  };
  std::vector<int>& live = run.live;
  int64_t it_done = 0;
  while (!live.empty() && it_done < n_points) {
    int64_t C = std::min<int64_t>(PLAN_CHUNK, n_points - it_done);
    if (refresh > 0) C = std::min<int64_t>(C, refresh - it_done % refresh);
    std::vector<mfgp_model*> lm;
    std::vector<int64_t> lk, loff;
    std::vector<int> lvi;
    std::vector<PlanMember> hm;
    int64_t liveM = 0, liveN = 0;
    for (int b : live) {
      if ((rc = run.grow(t[b], C))) return run.fail(rc);
      if (refresh > 0 && it_done > 0 && it_done % refresh == 0 && (rc = numerators(b))) return run.fail(rc);
      hm.push_back(describe(b, (int)lm.size()));
      lm.push_back(t[b]);
      lk.push_back(1);
      loff.push_back(moff[b]);
      lvi.push_back(b);
      liveM = std::max(liveM, t[b]->M);
      liveN = std::max(liveN, N0[b]);
    }
    const int nl = (int)lm.size();
    if (hipMemcpyAsync(dm, hm.data(), sizeof(PlanMember) * nl, hipMemcpyHostToDevice, s) != hipSuccess)
      return run.fail(set_err(MFGP_ERR_DEVICE, "%s: upload failed", who));
    for (int64_t it = 0; it < C; ++it) {
      if (launch_ivr_pick_batch(dm, nl, s) != hipSuccess)
        return run.fail(set_err(MFGP_ERR_DEVICE, "%s: launch failed", who));
      if (nl == count)
        rc = batch_run(lm.data(), count, xn, yn, lk.data(), mu, var, vmax, vargmax, MFGP_ASYNC, true, true);
      else
        rc = batch_run(lm.data(), nl, xn, yn, lk.data(), mu, var, vmax, vargmax, MFGP_ASYNC, true, true, loff.data(),
                       lvi.data());
      if (rc) return run.fail(rc);
      if (it_done + it + 1 >= n_points) break;   // the last pick: no score is read after it
      if (launch_plan_update_batch(dm, nl, it_done + it, liveM, liveN + it_done + it + 1, any_sep, s) != hipSuccess)
        return run.fail(set_err(MFGP_ERR_DEVICE, "%s: launch failed", who));
    }
    it_done += C;
    if ((rc = run.chunk_end())) return run.fail(rc);
    std::vector<int> keep;
    for (int b : live)
      if ((int)run.st[2 * b] != 0) keep.push_back(b);
    live.swap(keep);
  }
  for (int b = 0; b < count; ++b) {
    const int64_t n = counts[b] = run.st[2 * b + 1];
    if (n > 0 && (hipMemcpy(cells + b * P, dcells + b * P, sizeof(int64_t) * n, hipMemcpyDeviceToHost) != hipSuccess ||
                  hipMemcpy(gains + b * P, dgains + b * P, sizeof(double) * n, hipMemcpyDeviceToHost) != hipSuccess ||
                  hipMemcpy(points + 2 * b * P, dpts + 2 * b * P, sizeof(double) * 2 * n, hipMemcpyDefault) != hipSuccess ||
                  (pos && hipMemcpy(pos + b * P, dpos + b * P, sizeof(int64_t) * n, hipMemcpyDeviceToHost) != hipSuccess)))
      return run.fail(set_err(MFGP_ERR_DEVICE, "%s: copy out failed", who));
  }
  // (the posteriors' restore copies read ws)
  return run.finish(true) == MFGP_OK ? MFGP_OK : set_err(MFGP_ERR_DEVICE, "%s: restore failed", who);
}

extern "C" {

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
  // the reference works on a deep copy (sim:339); here on the model itself, brought
  // back to its own rows and state at the end (plan_enter / plan_leave)
  mfgp_model* t = model;
  if ((rc = plan_ready(c, &t, 1))) return rc;
  const int64_t M = t->M;
  // the context's workspace: mu, var [M] | vmax, vargmax, state {gate, count} | points [max_points][2] |
  // the saved resident posterior
  WsLayout lay;
  const size_t o_mu = lay.take(sizeof(double) * M), o_var = lay.take(sizeof(double) * M);
  const size_t o_misc = lay.take(sizeof(double) * 4);
  const size_t o_pts = lay.take(sizeof(double) * 2 * (size_t)std::max<int64_t>(max_points, 1));
  const size_t o_res = lay.take(sizeof(double) * plan_res_doubles(t));
  if ((rc = ensure_ws(c, lay.end))) return rc;
  PlanRun run("sample_points", c, &t, 1);
  run.ws = reinterpret_cast<char*>(c->ws.get());
  double *mu_s = run.at(o_mu), *var_s = run.at(o_var), *vmax = run.at(o_misc), *pts = run.at(o_pts);
  int64_t* vargmax = reinterpret_cast<int64_t*>(vmax + 1);
  run.state = vargmax + 1;
  int* gate = reinterpret_cast<int*>(run.state);
  if ((rc = run.enter(run.at(o_res)))) return run.fail(rc);
  // initial posterior (sim:340-342)
  if ((rc = batch_run(&t, 1, nullptr, nullptr, nullptr, mu_s, var_s, vmax, vargmax, 0, false, true))) return run.fail(rc);
  if (run.open() != hipSuccess) return run.fail(set_err(MFGP_ERR_DEVICE, "state upload failed"));
  bool active = true;
  while (active && run.done < max_points) {
    const int64_t C = std::min<int64_t>(PLAN_CHUNK, max_points - run.done);   // (two descriptors each)
    if ((rc = run.grow(t, C))) return run.fail(rc);
    int slot;
    GPDesc* hd = acquire_slot(c, slot, rc);
    if (!hd) return run.fail(rc);
    for (int64_t it = 0; it < C; ++it) {
      t->NH += 1;   // assume the iteration runs; truncated at the chunk's end if the loop stopped
      GPDesc& fd = hd[2 * it];
      if ((rc = fill_inc_desc(fd, t))) return run.fail(rc);
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
      t->st.predict_enqueued(Predict::VStream, t->NL + t->NH);
    }
    set_rsplit(c, hd + 1, 1);
    for (int64_t i = 0; i < 2 * C; ++i) hd[i].rsplit = hd[1].rsplit;
    const GPDesc* dd = nullptr;
    if ((rc = upload_slot(c, slot, (int)(2 * C), &dd))) return run.fail(rc);
    const int vf = t->dtype == MFGP_F32 ? 1 : 0;
    for (int64_t it = 0; it < C; ++it) {
      const bool ok = hipSuccess == launch_choi_select(dd + 2 * it, threshold, pts, max_points, c->stream) &&
                      (c->fused ? hipSuccess == launch_inc_stream(dd + 2 * it, 1,
                                                                   hd[2 * it].nprod + ntiles_wg(M, hd[2 * it].rsplit, vf),
                                                                   vf, c->stream)
                                : (hipSuccess == launch_inc_stream(dd + 2 * it, 1, hd[2 * it].nprod, vf, c->stream) &&
                                   hipSuccess == launch_vstream(dd + 2 * it + 1, 1, ntiles_wg(M, hd[2 * it + 1].rsplit, vf),
                                                                vf, c->stream)));
      if (!ok) return run.fail(set_err(MFGP_ERR_DEVICE, "sample_points: launch failed"));
    }
    if ((rc = release_slot(c, slot))) return run.fail(rc);
    if ((rc = run.chunk_end(C))) return run.fail(rc);
    active = (int)run.st[0] != 0;
  }
  if (run.done > 0 && hipMemcpy(points, pts, sizeof(double) * 2 * run.done, hipMemcpyDefault) != hipSuccess)
    return run.fail(set_err(MFGP_ERR_DEVICE, "sample_points: copy out failed"));
  *count = run.done;
  return run.finish(true);   // (the posterior's restore copy: ws is reused by the next call)
}

// compute_sample_points for a batch of models (the Choi planner's sample-set
// selection of many seeds, sim:326-374) stepped together: per iteration ONE
// k_choi_select_batch (every model's decision from its fused max / argmax) and ONE
// batched append + predict of every model's chosen row through the general batch
// step -- the lattice step where the batch takes it (its kernels and the V stream's
// honour each model's device gate, so a model past its threshold skips the rest of
// the chunk) -- with one host synchronisation per PLAN_CHUNK iterations. Each model
// works on its own rows past its own (sim:339's deep copy: plan_enter / plan_leave bring
// it back); the chosen points are the single-model loop's, up to the rounding of the
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
  mfgp_model* const* t = models;
  if ((rc = plan_ready(c, t, count))) return rc;
  // device state: mu, var [sum M] | vmax [B] | vargmax [B] | state [B][2] | thr [B] | moff [B] |
  // Ms [B] | grids [B] | status words [B] | xn [B][2] | yn [B] | pos [B] | points [B][max_points][2] |
  // the models' saved resident posteriors
  std::vector<int64_t> moff(count), Ms(count);
  std::vector<const double*> grids(count);
  std::vector<const int*> stat(count);
  int64_t Mtot = 0;
  size_t nres = 0;
  for (int b = 0; b < count; ++b) {
    moff[b] = Mtot;
    Ms[b] = t[b]->M;
    Mtot += t[b]->M;
    nres += plan_res_doubles(t[b]);
    grids[b] = t[b]->grid;
    stat[b] = t[b]->status;
  }
  const size_t P = (size_t)std::max<int64_t>(max_points, 1);
  const size_t dM = sizeof(double) * (size_t)Mtot, d8 = 8 * (size_t)count;   // (d8: one 8-byte entry per model)
  WsLayout lay;
  const size_t o_mu = lay.take(dM), o_var = lay.take(dM), o_vmax = lay.take(d8), o_varg = lay.take(d8);
  const size_t o_state = lay.take(2 * d8), o_thr = lay.take(d8), o_moff = lay.take(d8), o_Ms = lay.take(d8);
  const size_t o_grids = lay.take(d8), o_stat = lay.take(d8), o_xn = lay.take(2 * d8), o_yn = lay.take(d8);
  const size_t o_pos = lay.take(sizeof(int) * count), o_pts = lay.take(2 * d8 * P);
  const size_t o_res = lay.take(sizeof(double) * nres);
  PlanRun run("batch_sample_points", c, t, count);
  if (!run.own(lay.end)) return set_err(MFGP_ERR_DEVICE, "batch_sample_points: out of memory");
  if ((rc = run.enter(run.at(o_res)))) return run.fail(rc);
  double *mu = run.at(o_mu), *var = run.at(o_var), *vmax = run.at(o_vmax), *thr = run.at(o_thr);
  double *xn = run.at(o_xn), *yn = run.at(o_yn), *pts = run.at(o_pts);
  int64_t *vargmax = run.at<int64_t>(o_varg), *state = run.state = run.at<int64_t>(o_state);
  int64_t *moff_d = run.at<int64_t>(o_moff), *Ms_d = run.at<int64_t>(o_Ms);
  const double** grids_d = run.at<const double*>(o_grids);
  const int** stat_d = run.at<const int*>(o_stat);
  int* pos_d = run.at<int>(o_pos);
  hipStream_t s = c->stream;
  if (run.open() != hipSuccess ||
      hipMemcpyAsync(thr, thresholds, sizeof(double) * count, hipMemcpyDefault, s) != hipSuccess ||
      hipMemcpyAsync(moff_d, moff.data(), sizeof(int64_t) * count, hipMemcpyHostToDevice, s) != hipSuccess ||
      hipMemcpyAsync(Ms_d, Ms.data(), sizeof(int64_t) * count, hipMemcpyHostToDevice, s) != hipSuccess ||
      hipMemcpyAsync(grids_d, grids.data(), sizeof(double*) * count, hipMemcpyHostToDevice, s) != hipSuccess ||
      hipMemcpyAsync(stat_d, stat.data(), sizeof(int*) * count, hipMemcpyHostToDevice, s) != hipSuccess)
    return run.fail(set_err(MFGP_ERR_DEVICE, "batch_sample_points: state upload failed"));
  // the initial posteriors and their max / argmax (sim:340-342)
  if ((rc = batch_run(const_cast<mfgp_model**>(t), count, nullptr, nullptr, nullptr, mu, var, vmax, vargmax, 0,
                      false, true)))
    return run.fail(rc);
  for (int b = 0; b < count; ++b) t[b]->gate_dev = reinterpret_cast<int*>(state + 2 * b);
  // run.live: the models still running (the batch step's members; a stopped one leaves
  // at the next chunk boundary), their offsets into mu / var and indices into vmax
  std::vector<int>& live = run.live;
  int64_t it_done = 0;
  const auto tp1 = std::chrono::steady_clock::now();
  while (!live.empty() && it_done < max_points) {
    const int64_t C = std::min<int64_t>(PLAN_CHUNK, max_points - it_done);
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
      return run.fail(set_err(MFGP_ERR_DEVICE, "batch_sample_points: upload failed"));
    for (int64_t it = 0; it < C; ++it) {
      if (launch_choi_select_batch(count, pos_d, state, stat_d, thr, vmax, vargmax, mu, moff_d, grids_d, Ms_d, xn, yn,
                                   pts, max_points, s) != hipSuccess)
        return run.fail(set_err(MFGP_ERR_DEVICE, "batch_sample_points: launch failed"));
      if ((int)lm.size() == count)
        rc = batch_run(lm.data(), count, xn, yn, lk.data(), mu, var, vmax, vargmax, MFGP_ASYNC, true, true);
      else
        rc = batch_run(lm.data(), (int)lm.size(), xn, yn, lk.data(), mu, var, vmax, vargmax, MFGP_ASYNC, true, true,
                       loff.data(), lvi.data());
      if (rc) return run.fail(rc);
    }
    it_done += C;
    if ((rc = run.chunk_end())) return run.fail(rc);
    std::vector<int> keep;
    for (int b : live)
      if ((int)run.st[2 * b] != 0) keep.push_back(b);
    live.swap(keep);
  }
  const auto tp2 = std::chrono::steady_clock::now();
  for (int b = 0; b < count; ++b) {
    counts[b] = run.st[2 * b + 1];
    if (counts[b] > 0 && hipMemcpy(points + 2 * (size_t)b * P, pts + 2 * (size_t)b * P, sizeof(double) * 2 * counts[b],
                                   hipMemcpyDefault) != hipSuccess)
      return run.fail(set_err(MFGP_ERR_DEVICE, "batch_sample_points: copy out failed"));
  }
  const bool left = run.finish(false) == MFGP_OK;
  const auto tp3 = std::chrono::steady_clock::now();
  auto us = [](std::chrono::steady_clock::duration dt) {
    return (int64_t)std::chrono::duration_cast<std::chrono::microseconds>(dt).count();
  };
  c->plan_stats[8] += us(tp1 - tp0);
  c->plan_stats[9] += us(tp2 - tp1);
  c->plan_stats[10] += us(tp3 - tp2);
  return left ? MFGP_OK : set_err(MFGP_ERR_DEVICE, "batch_sample_points: restore failed");
}

// The greedy integrated-variance planner for one model: plan_ivr_run's batch of one, its
// list the nc cells of cand (NULL: all M), no groups and no recorded positions.
int mfgp_plan_ivr(mfgp_model* model, const double* w, int64_t ldw, const int64_t* cand, int64_t nc,
                  int64_t n_points, double min_gain, int refresh, int64_t* cells, double* points, double* gains,
                  int64_t* count) {
  const Entry entry(model);
  if (entry.rc) return entry.rc;
  if (!count) return set_err(MFGP_ERR_ARG, "mfgp_plan_ivr: null count");
  const int64_t cand_off[2] = {0, nc};
  return plan_ivr_run("mfgp_plan_ivr", true, &model, 1, w, ldw, cand, cand_off, nullptr, nullptr, 0, n_points,
                      min_gain, refresh, cells, nullptr, points, gains, count);
}

// mfgp_plan_ivr for a batch of models stepped together, with per-group quotas on the picks
// (plan_ivr_run).
int mfgp_batch_plan_ivr(mfgp_model** models, int count, const double* w, int64_t ldw, const int64_t* cand,
                        const int64_t* cand_off, const int32_t* group, const int64_t* quota, int ngroups,
                        int64_t n_points, double min_gain, int refresh, int64_t* cells, int64_t* pos, double* points,
                        double* gains, int64_t* counts) {
  const char* who = "mfgp_batch_plan_ivr";
  const DeviceGuard dg_((models && count > 0 && models[0]) ? models[0]->ctx->device : -1);
  if (const int rc_ = settle((models && count > 0 && models[0]) ? models[0]->ctx : nullptr)) return rc_;
  if (count <= 0 || !models) return set_err(MFGP_ERR_ARG, "%s: count must be positive and models non-null", who);
  if (!counts) return set_err(MFGP_ERR_ARG, "%s: null counts", who);
  return plan_ivr_run(who, false, models, count, w, ldw, cand, cand_off, group, quota, ngroups, n_points, min_gain,
                      refresh, cells, pos, points, gains, counts);
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
