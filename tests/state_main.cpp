// Stand-alone check of the record of what a model's derived buffers hold
// (csrc/mfgp_state.h): compiled and run by tests/test_state.py with the host compiler and
// -fsanitize=address,undefined. The directed checks drive every event and read every
// predicate; the walk runs every sequence of at most 4 of the library's calls, as its
// host files spell them in events, next to a shadow of what the launches really wrote
// (row identities, hyperparameters, grid and factor lineage per buffer), and checks on
// every prefix the state's own rules and that no predicate a call acts on names rows
// the shadow does not hold. Prints "ok" and exits 0, or the failed checks.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "mfgp_state.h"

using namespace mfgp_state;

namespace {

int failures = 0;
#define CHECK(cond)                                              \
  do {                                                           \
    if (!(cond)) {                                               \
      if (++failures <= 20) std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
    }                                                            \
  } while (0)

constexpr int64_t KINC = 16;
constexpr int MAXD = 256;
const double HYP[2][NHYP] = {{0.16, -2.03, -0.63, 1e-4, -3.1, -1.52, -0.65, -5.0, -2.0},
                             {0.16, -2.03, -0.63, 1e-4, -3.1, -1.52, -0.65, -5.0, -2.5}};
constexpr double JIT = 1e-8;
int64_t blocks(int64_t N) { return (N + 1 + 63) / 64; }

// a model factored over N rows with a full predict behind it
ModelState predicted(int64_t N) {
  ModelState s;
  s.full_factor_enqueued(N, blocks(N), HYP[0], JIT);
  s.factor_checked(true);
  s.predict_enqueued(Predict::Full, N, s.res_out(-1));
  return s;
}
// ... and a lattice step of k rows on top (the store written through)
void lattice_step(ModelState& s, int64_t N, int64_t k) {
  const int bin = s.res_find(N);
  CHECK(bin >= 0);
  s.compact_rows_written(N, N + k);
  s.inc_factor_enqueued(N + k, blocks(N + k));
  s.predict_enqueued(Predict::Lattice, N + k, 1 - bin, s.res[bin].depth + 1, true);
}

void test_tags() {
  RowTag t;
  CHECK(t.rows(0) == 0 && t.rows(1) == 0);
  t.set(7, 3);
  CHECK(t.rows(3) == 7 && t.rows(4) == 0);
  t.clamp(9);
  CHECK(t.rows(3) == 7);
  t.clamp(5);
  CHECK(t.rows(3) == 5);
  t.drop();
  CHECK(t.rows(3) == 0 && t.gen == 3);
  PostTag p;
  CHECK(!p.holds(0, 0) && p.n == -1);
  p.n = 0;   // the prior is a posterior of 0 rows
  CHECK(p.holds(0, 0));
  p.n = 6;
  p.clamp(6);
  CHECK(p.holds(6, 0));
  p.clamp(5);
  CHECK(p.n == -1);
}

// every writer, then every reader
void test_writers_and_readers() {
  ModelState s;
  CHECK(s.gen == 1 && !s.factored && s.v_n == 0 && s.res_find(0) == -1);
  CHECK(!s.factor_current(0, HYP[0], JIT) && !s.can_inc_factor(3, HYP[0], JIT, true, KINC));
  CHECK(s.lat_fbuild(0) && s.lat_axbuild() && s.tab_lo(5) == 0 && s.vcol_rows() == 0 && !s.l21c_ok(0));

  s.full_factor_enqueued(56, blocks(56), HYP[0], JIT);
  CHECK(s.gen == 2 && s.factored && s.factor_N == 56 && s.ablk == 1 && s.v_n == 0 && s.l21c_N == -1);
  s.factor_checked(true);
  CHECK(s.factor_current(56, HYP[0], JIT) && !s.factor_current(57, HYP[0], JIT));
  CHECK(!s.factor_current(56, HYP[1], JIT) && !s.factor_current(56, HYP[0], 2 * JIT));
  CHECK(!s.v_covers(56, HYP[0], JIT) && s.v_at_factor() == false);
  CHECK(s.can_inc_factor(59, HYP[0], JIT, true, KINC) && s.can_inc_factor(72, HYP[0], JIT, true, KINC));
  CHECK(!s.can_inc_factor(73, HYP[0], JIT, true, KINC) && !s.can_inc_factor(59, HYP[0], JIT, false, KINC));
  CHECK(!s.can_inc_factor(56, HYP[0], JIT, true, KINC) && !s.can_inc_factor(59, HYP[1], JIT, true, KINC));
  CHECK(s.can_vstream(16, KINC) && !s.can_vstream(17, KINC));

  CHECK(s.res_out(-1) == 0 && s.res_out(0) == 1 && s.res_out(1) == 0);
  s.predict_enqueued(Predict::Full, 56, 0);
  CHECK(s.v_n == 56 && s.v_covers(56, HYP[0], JIT) && s.v_at_factor() && s.res_find(56) == 0 && s.res_find(55) == -1);
  CHECK(s.res[0].depth == 0 && s.res[0].tick == 1 && s.tick == 1 && s.res_out(-1) == 1);
  CHECK(s.can_vstream(56, KINC) && s.can_vstream(72, KINC) && !s.can_vstream(73, KINC) && !s.can_vstream(55, KINC));
  CHECK(s.lat_depth_ok(56, MAXD) && !s.lat_depth_ok(55, MAXD) && !s.lat_depth_ok(56, 0));

  // a lattice step of 3 rows, the store written through
  s.compact_rows_written(56, 59);
  s.inc_factor_enqueued(59, blocks(59));
  CHECK(s.factor_N == 59 && s.ablk == 1 && s.l21c_n0 == 56 && s.l21c_N == 59);
  CHECK(s.l21c_ok(59) && !s.l21c_ok(60));   // (v_n is still 56: a one-pass predict may read the compact rows)
  s.predict_enqueued(Predict::Lattice, 59, 1, 1, true);
  CHECK(s.v_n == 59 && s.res_find(59) == 1 && s.res_find(56) == 0 && s.res[1].depth == 1 && s.res_out(-1) == 0);
  CHECK(!s.lat_fbuild(59) && !s.lat_fbuild(3) && s.lat_fbuild(60) && !s.lat_axbuild());
  CHECK(s.tab_lo(59) == 59 && s.tab_lo(40) == 40 && s.tab_lo(70) == 59 && s.vcol_rows() == 59);
  CHECK(!s.l21c_ok(59));   // (written for v_n = 56)
  CHECK(s.vcol_keep(true, 128, 64) == 59 && s.vcol_keep(true, 32, 64) == 32 && s.vcol_keep(false, 128, 64) == 0);
  CHECK(s.lat_depth_ok(59, 2) && !s.lat_depth_ok(59, 1));
  // without a store nothing is tagged for one; a V-stream predict leaves the store behind V
  ModelState u = predicted(56);
  lattice_step(u, 56, 3);
  u.vcol_reallocated();
  u.compact_rows_written(59, 62);
  u.inc_factor_enqueued(62, blocks(62));
  u.predict_enqueued(Predict::Lattice, 62, 0, 2, false);
  CHECK(u.vcol_rows() == 0 && u.F.rows(u.gen) == 62);
  u.vcol_rows_kept(40);
  CHECK(u.vcol_rows() == 40);
  u.predict_enqueued(Predict::VStream, 65, u.res_out(-1));
  CHECK(u.v_n == 65 && u.vcol_rows() == 40 && u.F.rows(u.gen) == 62 && u.res[1].depth == 0);
  u.predict_enqueued(Predict::Full, 65);   // a full predict rewrote V: the store starts over
  CHECK(u.vcol_rows() == 0 && u.tick == 4);   // (no posterior buffer written: no tick)

  // the factor_lost subsets stay different
  const ModelState base = s;
  const FactorLost only_factored[3] = {FactorLost::NotIncremental, FactorLost::RowsReplaced, FactorLost::StepFailed};
  for (int i = 0; i < 3; ++i) {
    ModelState a = base;
    a.factor_lost(only_factored[i]);
    CHECK(!a.factored && a.factor_N == 59 && a.ablk == 1 && a.v_n == 59 && a.l21c_N == 59 && a.gen == base.gen);
    CHECK(a.lost == base.lost + (i == 0 ? 0 : 1));
    CHECK(!a.factor_current(59, HYP[0], JIT) && !a.can_inc_factor(62, HYP[0], JIT, true, KINC));
  }
  {
    ModelState a = base;
    a.factor_lost(FactorLost::AsyncFailed);
    CHECK(!a.factored && a.ablk == 1 && a.v_n == 59 && a.l21c_N == -1 && a.l21c_n0 == 56 && a.lost == base.lost + 1);
    a.v_dropped();
    CHECK(a.v_n == 0 && a.lost == base.lost + 2 && a.vcol_rows() == 0);
    a.v_dropped();   // (nothing left to lose)
    a.factor_lost(FactorLost::StepFailed);
    CHECK(a.lost == base.lost + 2);
  }
  {
    ModelState a = base;
    a.factor_lost(FactorLost::Reallocated);
    CHECK(!a.factored && a.ablk == 0 && a.v_n == 59 && a.l21c_N == 59 && a.lost == base.lost + 1);
  }
  {
    ModelState a = base;
    a.factor_checked(true);
    CHECK(a.factored && a.lost == base.lost);
    a.factor_checked(false);
    CHECK(!a.factored && a.lost == base.lost + 1);
  }
  // the reallocation events
  {
    ModelState a = base;
    a.f_reallocated();
    CHECK(a.lat_fbuild(1) && a.tab_lo(59) == 59);
    a.tab_reallocated();
    CHECK(a.tab_lo(59) == 0);
    a.compact_rows_reallocated();
    CHECK(a.l21c_N == -1);
    a.axt_reallocated();
    CHECK(a.lat_axbuild() && a.axt_gen == UINT64_MAX);
    a.res_reallocated();
    CHECK(a.res_find(59) == -1 && a.res_find(56) == -1 && a.res_find(0) == -1 && !a.lat_depth_ok(59, MAXD));
    a.vcol_reallocated();
    CHECK(a.vcol_rows() == 0 && a.vcol_keep(true, 128, 128) == 0);
    a.vcol_rows_kept(32);
    CHECK(a.vcol_rows() == 32);
  }
  // a clone adopts the factor and V, nothing else
  {
    ModelState c;
    c.adopt_factor(base);
    CHECK(c.factored && c.factor_N == 59 && c.ablk == 1 && c.factor_current(59, HYP[0], JIT) && c.v_n == 0);
    c.adopt_v(base);
    CHECK(c.v_n == 59 && c.v_covers(59, HYP[0], JIT) && c.gen == 1 && c.res_find(59) == -1 && c.lat_fbuild(1));
  }
}

// after new_generation the gen-tagged buffers report 0 rows while v_n keeps its value
void test_new_generation() {
  ModelState s = predicted(56);
  lattice_step(s, 56, 3);
  s.new_generation();   // mfgp_model_set_hyp
  CHECK(s.v_n == 59 && s.can_vstream(59, KINC));   // (V has no generation: the hyp test below guards it)
  CHECK(!s.factor_current(59, HYP[1], JIT) && !s.can_inc_factor(62, HYP[1], JIT, true, KINC) && !s.v_covers(59, HYP[1], JIT));
  CHECK(s.F.rows(s.gen) == 0 && s.tab.rows(s.gen) == 0 && s.vc.rows(s.gen) == 0 && s.vcol_rows() == 0);
  CHECK(s.lat_fbuild(1) && s.lat_axbuild() && s.tab_lo(59) == 0 && s.vcol_keep(true, 128, 128) == 0);
  CHECK(s.res_find(59) == -1 && s.res_find(56) == -1 && !s.lat_depth_ok(59, MAXD));
  // the full factor the hyp test forces drops V before anything reads it
  s.full_factor_enqueued(59, blocks(59), HYP[1], JIT);
  CHECK(s.v_n == 0 && s.factor_current(59, HYP[1], JIT));
  // a new grid says so itself
  ModelState g = predicted(56);
  g.v_dropped();
  g.new_generation();
  CHECK(g.v_n == 0 && g.factor_current(56, HYP[0], JIT) && g.res_find(56) == -1 && g.lost == 1);
}

// truncate to N, append back to the same count: no posterior and no store row beyond N is found
void test_truncate_append_back() {
  ModelState s = predicted(56);
  lattice_step(s, 56, 3);
  lattice_step(s, 59, 8);
  CHECK(s.res_find(67) >= 0 && s.res_find(59) >= 0 && s.vcol_rows() == 67);
  s.rows_cut(62);
  CHECK(s.factor_N == 62 && s.v_n == 62 && s.vcol_rows() == 62 && s.F.rows(s.gen) == 62 && s.tab_lo(67) == 62);
  CHECK(s.res_find(67) == -1 && s.res_find(62) == -1 && s.res_find(59) >= 0);
  CHECK(s.l21c_n0 == 59 && s.l21c_N == 67 && !s.l21c_ok(62));   // the compact rows' tag stays
  // 5 other rows: a bordered append and its one-pass predict
  CHECK(s.can_inc_factor(67, HYP[0], JIT, true, KINC) && !s.lat_depth_ok(62, MAXD));
  s.compact_rows_written(62, 67);
  s.inc_factor_enqueued(67, blocks(67));
  CHECK(s.res_find(67) == -1 && s.vcol_rows() == 62 && s.l21c_ok(67));
  s.predict_enqueued(Predict::VStream, 67, s.res_out(-1));
  CHECK(s.res_find(67) >= 0 && s.res[s.res_find(67)].depth == 0 && s.vcol_rows() == 62 && s.F.rows(s.gen) == 62);
  // an unfactored model's factor_N is left alone (mfgp_truncate clamps it only when factored)
  ModelState u = predicted(56);
  u.factor_lost(FactorLost::StepFailed);
  u.rows_cut(40);
  CHECK(u.factor_N == 56 && u.v_n == 40);
}

// the three differences between rows_cut and restore_from, each with both outcomes, the
// invariant, and the least-recently-written choice across a save and restore
void test_restore() {
  const ModelState saved = predicted(56);
  auto loop = [&](ModelState& s) {   // a planner's loop: two lattice steps past the model's rows
    lattice_step(s, 56, 1);
    lattice_step(s, 57, 1);
  };
  // 1: the compact rows' tag -- rows_cut keeps it, restore_from drops it
  {
    ModelState a = saved, b = saved;
    loop(a);
    loop(b);
    a.rows_cut(56);
    CHECK(a.l21c_N == 58 && a.l21c_n0 == 57);
    CHECK(b.restore_from(saved, 56, true));
    CHECK(b.l21c_N == -1);
  }
  // 2: the factor -- rows_cut clamps factor_N only when factored and never sets factored;
  // restore_from takes both from the save
  {
    ModelState a = saved, b = saved;
    loop(a);
    loop(b);
    a.factor_lost(FactorLost::NotIncremental);
    b.factor_lost(FactorLost::NotIncremental);   // (the loop's last step refactors: not a loss)
    a.rows_cut(56);
    CHECK(!a.factored && a.factor_N == 58);
    CHECK(b.restore_from(saved, 56, true));
    CHECK(b.factored && b.factor_N == 56 && b.factor_current(56, HYP[0], JIT));
    ModelState c = saved, d = saved;   // factored: the same clamp either way
    loop(c);
    loop(d);
    c.rows_cut(56);
    CHECK(d.restore_from(saved, 56, true));
    CHECK(c.factored && c.factor_N == 56 && d.factored && d.factor_N == 56);
  }
  // 3: V -- rows_cut takes min(v_n, N); restore_from the larger of that and the saved rows
  {
    ModelState a = saved, b = saved;
    loop(a);
    loop(b);
    a.full_factor_enqueued(58, blocks(58), HYP[0], JIT);   // (a loop with incremental off: V starts over)
    b.full_factor_enqueued(58, blocks(58), HYP[0], JIT);
    a.rows_cut(56);
    CHECK(a.v_n == 0);
    CHECK(b.restore_from(saved, 56, true));
    CHECK(b.v_n == 56);
    ModelState unpred;   // saved without V: what the loop's first predict built of the leading rows stays
    unpred.full_factor_enqueued(56, blocks(56), HYP[0], JIT);
    ModelState c = unpred;
    c.predict_enqueued(Predict::Full, 56, 0);
    lattice_step(c, 56, 2);
    CHECK(c.restore_from(unpred, 56, false));
    CHECK(c.v_n == 56 && c.res_find(56) == 0 && c.res_find(58) == -1);   // (no saved posterior: cut, as rows_cut)
  }
  // the invariant: a drop for real inside the loop, and restore_from refuses to resurrect
  for (int what = 0; what < 3; ++what) {
    ModelState b = saved;
    loop(b);
    if (what == 0) b.v_dropped();
    if (what == 1) b.factor_lost(FactorLost::Reallocated);
    if (what == 2) b.factor_lost(FactorLost::AsyncFailed);
    const ModelState before = b;
    CHECK(!b.restore_from(saved, 56, true));
    CHECK(b.factored == before.factored && b.v_n == std::min<int64_t>(before.v_n, 56) && b.l21c_N == -1);
    CHECK(b.res_find(58) == -1 && b.res_find(57) == -1 && b.F.rows(b.gen) == 56);
  }
  // the posterior: saved tags back, tick no older than either, and the next predict
  // writes the buffer written longest ago by the model's own predicts
  {
    ModelState s0 = predicted(56);                       // buffer 0 at tick 1
    s0.predict_enqueued(Predict::VStream, 56, s0.res_out(-1));   // buffer 1 at tick 2
    s0.predict_enqueued(Predict::VStream, 56, s0.res_out(-1));   // buffer 0 at tick 3
    CHECK(s0.res[0].tick == 3 && s0.res[1].tick == 2 && s0.res_out(-1) == 1);
    ModelState b = s0;
    loop(b);   // writes buffer 1 (tick 4), then buffer 0 (tick 5)
    CHECK(b.tick == 5 && b.res_out(-1) == 1);
    CHECK(b.restore_from(s0, 56, true));
    CHECK(b.tick == 5 && b.res[0].tick == 3 && b.res[1].tick == 2 && b.res_out(-1) == 1 && b.res_find(56) >= 0);
    b.predict_enqueued(Predict::VStream, 56, b.res_out(-1));
    CHECK(b.res[1].tick == 6 && b.res_out(-1) == 0);
    ModelState c = s0;   // a save newer than the state (tick = max)
    c.tick = 1;
    CHECK(c.restore_from(s0, 56, true));
    CHECK(c.tick == 3);
  }
}

// ---- the walk ----
// One model as the host files drive it. rows: the identities of its training rows. Each
// shadow buffer records what a launch wrote: the rows it covers and the hyperparameters,
// grid and factor lineage they were computed for.
struct Shadow {
  std::vector<int> ids;
  int hyp = -1, grid = -1, lineage = -1;
};
struct Sim {
  ModelState st;
  std::vector<int> rows;
  int next_id = 1, hyp = 0, grid = 0, lineage = 0;
  bool incremental = true;
  Shadow fac, V, F, tab, vc, res[2];
  int axt_hyp = -1, axt_grid = -1;
  int64_t findings = 0;

  int64_t N() const { return (int64_t)rows.size(); }
  bool prefix(const Shadow& b, int64_t n) const {   // b's first n rows are the model's
    if ((int64_t)b.ids.size() < n || N() < n) return false;
    for (int64_t i = 0; i < n; ++i)
      if (b.ids[i] != rows[i]) return false;
    return true;
  }
  void finding(bool ok) {
    if (!ok) ++findings;
  }
  void add_rows(int64_t k) {
    for (int64_t i = 0; i < k; ++i) rows.push_back(next_id++);
  }
  void write_rows(Shadow& b, int64_t from) {   // a launch wrote b's rows [from, N)
    b.ids.resize((size_t)from);
    for (int64_t i = from; i < N(); ++i) b.ids.push_back(rows[i]);
  }
  void full_factor() {
    st.full_factor_enqueued(N(), blocks(N()), HYP[hyp], JIT);
    write_rows(fac, 0);
    fac.hyp = hyp;
    fac.lineage = ++lineage;
  }
  void inc_factor() {   // fill_inc_desc + mark_inc_factor: rows [factor_N, N) bordered on
    finding(prefix(fac, st.factor_N) && fac.hyp == hyp);
    st.compact_rows_written(st.factor_N, N());
    write_rows(fac, st.factor_N);
    st.inc_factor_enqueued(N(), blocks(N()));
  }
  void update_factor() {
    if (st.factor_current(N(), HYP[hyp], JIT)) {
      finding(prefix(fac, N()) && fac.hyp == hyp);
      return;
    }
    if (st.can_inc_factor(N(), HYP[hyp], JIT, incremental, KINC)) inc_factor();
    else full_factor();
    st.factor_checked(true);
  }
  bool v_valid(int64_t n) const {
    return n == 0 || (prefix(V, n) && V.hyp == hyp && V.grid == grid && V.lineage == fac.lineage);
  }
  bool post_valid(const Shadow& b, int64_t n) const {
    return (int64_t)b.ids.size() == n && prefix(b, n) && b.hyp == hyp && b.grid == grid && b.lineage == fac.lineage;
  }
  void write_post(int b) {
    if (b < 0) return;
    write_rows(res[b], 0);
    res[b].hyp = hyp;
    res[b].grid = grid;
    res[b].lineage = fac.lineage;
  }
  // the predict of a current factor: one pass over V where it serves, else the full one
  void predict_current() {
    const bool vst = incremental && st.can_vstream(N(), KINC);
    const int rb = incremental ? st.res_out(-1) : -1;
    if (vst) {
      finding(v_valid(st.v_n));
      if (st.v_n == 0) V = Shadow{{}, hyp, grid, fac.lineage};
      write_rows(V, st.v_n);
    } else {
      V = Shadow{{}, hyp, grid, fac.lineage};
      write_rows(V, 0);
    }
    st.predict_enqueued(vst ? Predict::VStream : Predict::Full, N(), rb);
    write_post(rb);
  }
  void set_data(int64_t n) {
    rows.clear();
    add_rows(n);
    st.factor_lost(FactorLost::RowsReplaced);
    full_factor();
    st.factor_checked(true);
  }
  void append(int64_t k) {   // mfgp_append, not speculative
    add_rows(k);
    if (!incremental) st.factor_lost(FactorLost::NotIncremental);
    update_factor();
  }
  void predict() {
    update_factor();
    predict_current();
  }
  // the batch step of one model: k rows and a predict (serve_unchanged, sub_batch)
  void step(int64_t k) {
    if (k == 0 && incremental && st.factor_current(N(), HYP[hyp], JIT) && st.v_n == N()) {
      const int b = st.res_find(N());
      if (b >= 0) {   // k_post_copy
        finding(post_valid(res[b], N()));
        return;
      }
    }
    add_rows(k);
    if (!incremental) st.factor_lost(FactorLost::NotIncremental);
    const bool inc = !st.factor_current(N(), HYP[hyp], JIT) && st.can_inc_factor(N(), HYP[hyp], JIT, incremental, KINC);
    const int64_t n0 = st.factor_N;
    if (inc) inc_factor();
    else if (!st.factor_current(N(), HYP[hyp], JIT)) full_factor();
    const bool fuse = inc && incremental && st.can_vstream(N(), KINC) && n0 == st.v_n;
    if (fuse && n0 >= 1 && st.lat_depth_ok(n0, MAXD)) {
      const int bin = st.res_find(n0);
      finding(post_valid(res[bin], n0) && v_valid(n0));
      if (!st.lat_fbuild(n0)) finding(prefix(F, n0) && F.hyp == hyp && F.lineage == fac.lineage);
      if (!st.lat_axbuild()) finding(axt_hyp == hyp && axt_grid == grid);
      finding(prefix(tab, st.tab_lo(n0)) && (st.tab_lo(n0) == 0 || (tab.hyp == hyp && tab.grid == grid)));
      const int64_t vlo = std::min(st.vcol_rows(), n0);
      finding(vlo == 0 || (prefix(vc, vlo) && vc.hyp == hyp && vc.grid == grid && vc.lineage == fac.lineage));
      F = Shadow{{}, hyp, -1, fac.lineage};
      write_rows(F, 0);
      tab = Shadow{{}, hyp, grid, -1};
      write_rows(tab, 0);
      vc = Shadow{{}, hyp, grid, fac.lineage};
      write_rows(vc, 0);
      axt_hyp = hyp;
      axt_grid = grid;
      write_rows(V, n0);
      st.predict_enqueued(Predict::Lattice, N(), 1 - bin, st.res[bin].depth + 1, true);
      write_post(1 - bin);
      return;
    }
    predict_current();
  }
  void truncate(int64_t n) {
    if (n >= N()) return;
    rows.resize((size_t)n);
    st.rows_cut(n);
  }
  void set_hyp() {
    hyp ^= 1;
    st.new_generation();
  }
  void set_grid() {
    ++grid;
    st.v_dropped();
    st.new_generation();
  }
  void grow() {   // ensure_cap past the capacity: the factor's buffers move with their contents where it is served
    const bool keep = st.factored && st.ablk > 0;
    if (!keep || st.F.n == 0) {
      F = Shadow{};
      st.f_reallocated();
    }
    if (st.tab.n == 0) {
      tab = Shadow{};
      st.tab_reallocated();
    }
    st.compact_rows_reallocated();
    if (!keep) {
      fac = Shadow{};
      st.factor_lost(FactorLost::Reallocated);
      st.v_dropped();
    }
  }
  void async_failed() {   // mfgp_ctx_synchronize reads a failed status word of this model
    fac = Shadow{};
    st.factor_lost(FactorLost::AsyncFailed);
    st.v_dropped();
  }
  void plan() {   // a planner's loop of one row on the model in place (plan_ready, enter, step, leave)
    update_factor();
    const ModelState saved = st;
    const Shadow r0 = res[0], r1 = res[1];
    const int64_t n = N();
    step(1);
    rows.resize((size_t)n);
    const bool kept = st.restore_from(saved, n, true);
    CHECK(kept);
    res[0] = r0;
    res[1] = r1;
  }

  // the state's own rules, on every prefix
  void check_rules() {
    const int64_t n = N();
    CHECK(!st.factored || st.factor_N <= n);
    CHECK(st.v_n <= n && st.F.rows(st.gen) <= n && st.tab.rows(st.gen) <= n && st.vc.rows(st.gen) <= n && st.vcol_rows() <= n);
    CHECK(st.tab_lo(n + 3) <= n && st.vcol_keep(true, 64, 64) <= n);
    for (int64_t q = 0; q <= n + 4; ++q) {   // (every caller asks for a row count)
      const int b = st.res_find(q);
      CHECK(b < 0 || (st.res[b].gen == st.gen && st.res[b].n == q && q <= n));
    }
    CHECK(st.res[0].tick <= st.tick && st.res[1].tick <= st.tick);
    if (st.factor_current(n, HYP[hyp], JIT)) finding(prefix(fac, n) && fac.hyp == hyp);
  }
};

constexpr int NEVENTS = 16;
const char* const EVENT_NAME[NEVENTS] = {"set_data(0)", "set_data(5)", "set_data(8)", "append(0)", "append(3)", "predict",
                                         "step(3)", "step(0)", "truncate(0)", "truncate(5)", "truncate(8)", "set_hyp",
                                         "set_grid", "grow", "async_failed", "plan"};
void apply(Sim& s, int e) {
  switch (e) {
    case 0: s.set_data(0); break;
    case 1: s.set_data(5); break;
    case 2: s.set_data(8); break;
    case 3: s.append(0); break;
    case 4: s.append(3); break;
    case 5: s.predict(); break;
    case 6: s.step(3); break;
    case 7: s.step(0); break;
    case 8: s.truncate(0); break;
    case 9: s.truncate(5); break;
    case 10: s.truncate(8); break;
    case 11: s.set_hyp(); break;
    case 12: s.set_grid(); break;
    case 13: s.grow(); break;
    case 14: s.async_failed(); break;
    default: s.plan(); break;
  }
  // "no tag exceeds N after rows_cut(N)", for every N of the alphabet, on a copy
  const int64_t cuts[3] = {0, 5, 8};
  for (int64_t n : cuts) {
    ModelState c = s.st;
    c.rows_cut(n);
    CHECK((!c.factored || c.factor_N <= n) && c.v_n <= n && c.F.n <= n && c.tab.n <= n && c.vc.n <= n);
    CHECK(c.res[0].n <= n && c.res[1].n <= n);
  }
  s.check_rules();
}

// every sequence of 1 .. 4 events, from a model that was set up (8 rows, predicted) and from
// one that was not; returns the sequences walked
int64_t walk(bool incremental) {
  int64_t sequences = 0, findings = 0;
  for (int start = 0; start < 2; ++start) {
    Sim root;
    root.incremental = incremental;
    if (start) {
      root.set_data(8);
      root.predict();
    }
    for (int len = 1; len <= 4; ++len) {
      int64_t total = 1;
      for (int i = 0; i < len; ++i) total *= NEVENTS;
      for (int64_t code = 0; code < total; ++code) {
        Sim s = root;
        int64_t c = code;
        int ev[4] = {0, 0, 0, 0};
        for (int i = 0; i < len; ++i, c /= NEVENTS) apply(s, ev[i] = (int)(c % NEVENTS));
        ++sequences;
        if (s.findings && ++findings <= 5) {
          std::printf("FINDING (%s, incremental %d):", start ? "predicted model" : "new model", (int)incremental);
          for (int i = 0; i < len; ++i) std::printf(" %s", EVENT_NAME[ev[i]]);
          std::printf("\n");
        }
      }
    }
  }
  CHECK(findings == 0);
  return sequences;
}

}  // namespace

int main() {
  test_tags();
  test_writers_and_readers();
  test_new_generation();
  test_truncate_append_back();
  test_restore();
  const int64_t n = walk(true) + walk(false);
  CHECK(n == 4 * (16 + 256 + 4096 + 65536));
  if (failures) {
    std::printf("%d checks failed\n", failures);
    return 1;
  }
  std::printf("ok\n");
  return 0;
}
