// What a model's derived buffers hold, and the only code that changes it (plain C++, no
// HIP: mfgp_model holds one ModelState by value as `st`; tests/state_main.cpp drives it
// alone). The buffers themselves, their shapes and strides stay in mfgp_model; this is the
// host's record of which rows of each are current:
//
//   the factor      rows [0, factor_N) of A / Linv / zv, for factor_hyp / factor_jitter
//   V               rows [0, v_n). V carries no generation: every event that invalidates
//                   it drops v_n (v_dropped, full_factor_enqueued) -- but for new
//                   hyperparameters, which leave v_n and rely on the factor's hyp test
//                   forcing a full factor (which then drops it) before V is read again
//   compact rows    the bordered rows [l21c_n0, l21c_N) in iscr
//   F, tab, vc      RowTag: rows [0, n) current for one generation (tab's also tags lidx)
//   axt             current for generation axt_gen
//   res[2]          PostTag: the posterior of exactly n leading rows, for one generation
//
// Writers are the named events below (nothing outside this header assigns a field);
// readers are const members taking what they need as plain numbers. The free functions
// of mfgp_host.h add the pointer and shape tests.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>

namespace mfgp_state __attribute__((visibility("hidden"))) {   // (no symbols of the library)

// rows [0, n) of a buffer, current for generation `gen`
struct RowTag {
  int64_t n = 0;
  uint64_t gen = 0;
  int64_t rows(uint64_t g) const { return gen == g ? n : 0; }
  void set(int64_t n_, uint64_t g) {
    n = n_;
    gen = g;
  }
  void clamp(int64_t N) { n = std::min(n, N); }
  void drop() { n = 0; }
};

// One of the two resident posterior buffers: [mu | var] of exactly the n leading rows (a
// posterior is no prefix of a longer one: cutting rows drops it; -1: none -- 0 rows is
// the prior, a posterior like any other), `depth` lattice steps since var / mu were
// computed from V, written at `tick`.
struct PostTag {
  int64_t n = -1;
  uint64_t gen = 0;
  int depth = 0;
  uint64_t tick = 0;
  // (callers ask for a row count; n_ = -1 would match a dropped tag of generation g, as it always did)
  bool holds(int64_t n_, uint64_t g) const { return n == n_ && gen == g; }
  void clamp(int64_t N) {
    if (n > N) drop();
  }
  void drop() { n = -1; }
};

enum class Predict { Full, VStream, Lattice };

// Why a factor is no longer served. Each clears what its site always cleared; the subsets
// differ on purpose (the sites that also lose V say so with v_dropped()).
enum class FactorLost {
  NotIncremental,   // reference behaviour, every update refactors: `factored` (the device's factor is sound)
  RowsReplaced,     // mfgp_set_data: `factored`
  StepFailed,       // a synchronous factor or step reported failure: `factored`
  AsyncFailed,      // a deferred status word reported failure: `factored`, the compact rows
  Reallocated       // A / Linv / zv replaced without their contents: `factored`, `ablk`
};

constexpr int NHYP = 9;

struct ModelState {
  // state generation: a new factor from scratch, a new grid or new hyperparameters start
  // a new one (the resident posterior, F, the tables and the column store belong to one)
  uint64_t gen = 1;
  bool factored = false;
  int64_t factor_N = -1;    // rows [0, factor_N) of A / Linv / zv hold the current factor
  int64_t ablk = 0;         // 64-row blocks of A / Linv initialised (assembled or padded)
  double factor_hyp[NHYP] = {0};
  double factor_jitter = 0.0;
  int64_t v_n = 0;          // rows [0, v_n) of V valid for the current factor and grid
  int64_t l21c_n0 = -1, l21c_N = -1;   // (-1: none)
  RowTag F, tab, vc;
  uint64_t axt_gen = 0;
  PostTag res[2];
  uint64_t tick = 0;
  // events that lost a served factor or rows of V for real (every FactorLost but
  // NotIncremental of a factored model, v_dropped of a V with rows): what restore_from's
  // invariant watches. Kept in every build, not only debug ones: an increment per loss and one
  // compare per planner call, so that a release build refuses to resurrect a lost factor too
  uint64_t lost = 0;

  // ---- events ----
  void new_generation() { gen += 1; }
  void v_dropped() {
    if (v_n > 0) lost += 1;
    v_n = 0;
  }
  void factor_lost(FactorLost what) {
    if (factored && what != FactorLost::NotIncremental) lost += 1;
    factored = false;
    if (what == FactorLost::AsyncFailed) l21c_N = -1;
    if (what == FactorLost::Reallocated) ablk = 0;
  }
  // the verdict of a synchronous factor launch (factor_one, update_factor)
  void factor_checked(bool ok) {
    if (!ok) factor_lost(FactorLost::StepFailed);
  }
  // a factor from scratch over N rows (`blocks`: its 64-row blocks): new rounding of
  // everything derived from it, and V belonged to the previous factor
  void full_factor_enqueued(int64_t N, int64_t blocks, const double* hyp, double jitter) {
    new_generation();
    factored = true;
    factor_N = N;
    std::memcpy(factor_hyp, hyp, sizeof(factor_hyp));
    factor_jitter = jitter;
    ablk = std::max(ablk, blocks);
    v_n = 0;
    l21c_N = -1;
  }
  void inc_factor_enqueued(int64_t N, int64_t blocks) {
    factor_N = N;
    ablk = std::max(ablk, blocks);
  }
  // the producers of a bordered append write the compact rows for (n0, N)
  void compact_rows_written(int64_t n0, int64_t N) {
    l21c_n0 = n0;
    l21c_N = N;
  }
  // A predict over N rows is enqueued: V holds them. res_b >= 0: it writes that posterior
  // buffer. A full predict rewrote V, so the column store starts over; a lattice step
  // (`depth`: the written buffer's) brought F's new rows, the new rows' tables and the axis
  // tables with it, and wrote the store through where it has one (vcol_written).
  void predict_enqueued(Predict kind, int64_t N, int res_b = -1, int depth = 0, bool vcol_written = false) {
    v_n = N;
    if (kind == Predict::Full) vc.drop();
    if (res_b >= 0) {
      res[res_b].n = N;
      res[res_b].gen = gen;
      res[res_b].depth = kind == Predict::Lattice ? depth : 0;
      res[res_b].tick = ++tick;
    }
    if (kind != Predict::Lattice) return;
    F.set(N, gen);
    if (vcol_written) vc.set(N, gen);
    tab.set(N, gen);
    axt_gen = gen;
  }
  // Rows cut to N (mfgp_truncate): the factor, z, V, F, the tables and the store of the
  // leading rows do not depend on later rows; the posterior of rows that are gone goes.
  // The compact rows' tag stays (l21c_ok compares it with N).
  void rows_cut(int64_t N) {
    if (factored && factor_N > N) factor_N = N;
    v_n = std::min(v_n, N);
    F.clamp(N);
    vc.clamp(N);
    tab.clamp(N);
    for (PostTag& r : res) r.clamp(N);
  }
  // A planner's loop ends on a model it appended to in place: back to the N rows and the
  // state `saved` at its start. rows_cut, and where it differs:
  //   - the factor is the one saved, whatever the loop left (a failed step too): the loop
  //     wrote rows past N only
  //   - V keeps what the loop's first predict built of the leading rows, beyond the saved
  //   - the compact rows in iscr are the loop's: dropped
  //   - the posterior buffers were copied back (`posterior`): their saved tags, and a
  //     tick no older than either
  // INVARIANT: between the save and here nothing lost the factor or V's leading rows for
  // real (`lost` unchanged), or the first two would resurrect them. False: it did; the
  // state is cut to N and nothing is restored.
  bool restore_from(const ModelState& saved, int64_t N, bool posterior) {
    rows_cut(N);
    l21c_N = -1;
    if (lost != saved.lost) return false;
    factored = saved.factored;
    factor_N = std::min(saved.factor_N, N);
    v_n = std::max(v_n, std::min(saved.v_n, N));
    if (posterior) {
      for (int b = 0; b < 2; ++b) res[b] = saved.res[b];
      tick = std::max(tick, saved.tick);
    }
    return true;
  }
  // a buffer group replaced (ensure_cap, ensure_res, ensure_lat, ensure_vcol)
  void f_reallocated() { F.drop(); }
  void tab_reallocated() { tab.drop(); }
  void compact_rows_reallocated() { l21c_N = -1; }
  void axt_reallocated() { axt_gen = UINT64_MAX; }   // build before use
  void res_reallocated() {
    for (PostTag& r : res) r.drop();
  }
  void vcol_reallocated() { vc.drop(); }
  void vcol_rows_kept(int64_t keep) { vc.n = keep; }   // (of its own generation: vcol_keep)
  // mfgp_clone: the copy's factor / V are the source's
  void adopt_factor(const ModelState& src) {
    factored = true;
    factor_N = src.factor_N;
    ablk = src.ablk;
    std::memcpy(factor_hyp, src.factor_hyp, sizeof(factor_hyp));
    factor_jitter = src.factor_jitter;
  }
  void adopt_v(const ModelState& src) { v_n = src.v_n; }

  // ---- readers (hyp: the model's NHYP words, compared as bytes) ----
  bool hyp_same(const double* hyp, double jitter) const {
    return factor_jitter == jitter && std::memcmp(factor_hyp, hyp, sizeof(factor_hyp)) == 0;
  }
  bool factor_current(int64_t N, const double* hyp, double jitter) const {
    return factored && factor_N == N && hyp_same(hyp, jitter);
  }
  // rows [factor_N, N) can be appended to the current factor, at most kinc of them
  bool can_inc_factor(int64_t N, const double* hyp, double jitter, bool incremental, int64_t kinc) const {
    return incremental && factored && hyp_same(hyp, jitter) && factor_N < N && N - factor_N <= kinc;
  }
  // V valid for rows < v_n, at most kinc rows beyond it
  bool can_vstream(int64_t N, int64_t kinc) const { return v_n <= N && N - v_n <= kinc; }
  bool v_covers(int64_t N, const double* hyp, double jitter) const { return factor_current(N, hyp, jitter) && v_n == N; }
  // the eager append's speculative step: V resident up to the factor
  bool v_at_factor() const { return v_n == factor_N; }
  // the buffer holding the posterior of the n leading rows (-1: none)
  int res_find(int64_t n) const {
    for (int b = 0; b < 2; ++b)
      if (res[b].holds(n, gen)) return b;
    return -1;
  }
  // the buffer a predict writes: not `keep`, else the least recently written
  int res_out(int keep) const {
    if (keep >= 0) return 1 - keep;
    return res[0].tick <= res[1].tick ? 0 : 1;
  }
  // the lattice step from n0 rows reads a resident posterior less than maxd steps deep
  bool lat_depth_ok(int64_t n0, int maxd) const {
    const int b = res_find(n0);
    return b >= 0 && res[b].depth < maxd;
  }
  bool lat_fbuild(int64_t n0) const { return !(F.gen == gen && F.n >= n0); }
  bool lat_axbuild() const { return axt_gen != gen; }
  int64_t tab_lo(int64_t n0) const { return std::min(tab.rows(gen), n0); }
  // the compact rows serve a one-pass predict over V's rows when the last bordered append
  // wrote them for exactly these rows
  bool l21c_ok(int64_t N) const { return l21c_n0 == v_n && l21c_N == N; }
  // rows of the store that equal V's now
  int64_t vcol_rows() const { return vc.gen == gen ? std::min(vc.n, v_n) : 0; }
  // rows of the old store that stay valid in a new one of stride ldc (same_grid: the old
  // one's cells are the grid's)
  int64_t vcol_keep(bool same_grid, int64_t ldc, int64_t old_ld) const {
    return (vc.gen == gen && same_grid) ? std::min({vc.n, v_n, ldc, old_ld}) : 0;
  }
};

}  // namespace mfgp_state
