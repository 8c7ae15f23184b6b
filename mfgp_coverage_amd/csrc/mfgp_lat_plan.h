// The arithmetic of the lattice step's launch plan (mfgp_step.hip: plan_lat), on plain
// numbers: whether the step is worth taking, its GEMM as a second launch or as
// in-launch split-K tiles, the split, the w units of the launch and each GP's share.
// Standard library only, so that a host test compiles and calls the rule that runs
// (tests/lat_plan_main.cpp).
#pragma once
#include <algorithm>
#include <cstdint>

namespace mfgp_lat_plan __attribute__((visibility("hidden"))) {

constexpr int WU_MAX = 512;   // w units per GP (mfgp_internal.h: LAT_WU_MAX)
constexpr int KSTAGE = 8;     // K rows per pipeline stage of the GEMM (mfgp_internal.h: ZKS)

// the context's part: the chip and the override knobs (mfgp_ctx)
struct Knobs {
  int ncu;           // compute units
  int lat_gemm2;     // -1: by the tile count, 1 always, 0 never
  bool concurrent;   // launches may share the chip with other contexts'
  bool lat_force;    // take the step whatever it costs
  int lat_ksplit;    // > 0: this split-K
  int lat_wu;        // > 0: this many w units over the launch
};
// one GP of the step
struct Gp {
  int64_t n0;   // factor rows before the step
  int64_t k;    // new rows
  int64_t M;    // grid cells
  int es;       // bytes of an element of V
  int nx, ny;   // the lattice
  bool sf;      // single fidelity
};
struct Plan {
  bool take;            // false: the V stream is cheaper
  int ka;               // new-row slots of the GEMM's tiles (8 or 16)
  bool g2;              // the GEMM and cells as a second launch
  int ksplit;           // split-K of the in-launch tiles
  int64_t tiles_sum;    // GEMM tiles of the launch
  int64_t wsteps_sum;   // F steps of the launch
  int64_t wu_total;     // w units of the launch
};

// 16-row steps of F's lower triangle over n0 rows (mfgp_internal.h: lat_wsteps)
inline int64_t wsteps(int64_t n0) {
  const int64_t C = (n0 + 15) / 16, nwb = (n0 + 63) / 64;
  return nwb * C - 2 * nwb * (nwb - 1);
}
// in-launch GEMM tiles: 128 (a, ix) rows x 64 iy columns
inline int64_t tiles(int nx, int ny, int ka) { return ((nx + 128 / ka - 1) / (128 / ka)) * ((ny + 63) / 64); }
// k_lat_gemm2's tiles: 64 (a, ix) rows x 64 iy columns
inline int64_t tiles2(int nx, int ny, int ka) { return ((nx + 64 / ka - 1) / (64 / ka)) * ((ny + 63) / 64); }

// the GEMM as a second launch (k_lat_gemm2: no split-K partials through memory,
// no hand-off flags) where its tiles fill the chip once or twice: at the
// headline (B = 8, 256 tiles) 80 vs 100 us per step; a batch of many more tiles
// (configs[4]: 4096) keeps the in-launch tiles, whose GEMM overlaps the other
// GPs' F streams (2.35 vs 3.05 ms per step), and so does one GP (52 vs 57 us)
inline bool second_launch(const Knobs& c, int64_t t2) {
  bool g2 = c.lat_gemm2 > 0 || (c.lat_gemm2 < 0 && t2 >= c.ncu && t2 <= 2 * (int64_t)c.ncu);
  // (split-K tiles of one launch wait for each other: they need the whole chip)
  if (c.concurrent) g2 = true;
  return g2;
}

// the lattice step has a fixed cost (its chain of dependent phases) plus the F
// stream and the GEMM (~0.8 us per million n0^2); the V stream reads 8 n0 M
// bytes per GP (~5.5 TB/s) -- measured at 128x128, N = 2048 (us per step, V
// stream / lattice with the second-launch GEMM, round 3): B = 8 345 / 80; B = 1
// 60 / 57 back to back; in the drop-in step (one GP, the eager append returning
// at the L22 verdict, round 5: tools/bench_dropin.py) 93.2 / 88.3-90.3 us, so
// the fixed cost is priced at 50 and one GP from n0 ~ 1700 (at M = 16384) takes
// the lattice; configs[4] (32 GPs, 256x256, N = 8192, fp32 V) 11.2 / 2.4 ms
inline bool cheaper_than_vstream(const Gp* g, int n) {
  double vs_us = 10.0, lat_us = 50.0;
  for (int i = 0; i < n; ++i) {
    const double n0 = (double)g[i].n0, es = g[i].es == 4 ? 4.0 : 8.0;
    vs_us += (double)g[i].M * n0 * es / 5.5e6;
    lat_us += 0.81 * n0 * n0 / 1.0e6;
  }
  return !(lat_us >= vs_us);
}

// split-K so that the GEMM tiles fill the chip about twice, >= 4 stages each
// (the second-launch GEMM splits K inside its workgroups: S = 1 here)
inline int split_k(const Knobs& c, bool g2, int64_t tiles_sum, int64_t nst_min) {
  int S = (int)std::min<int64_t>(8, std::max<int64_t>(1, (2 * c.ncu + tiles_sum - 1) / tiles_sum));
  if (g2) S = 1;
  // (split s takes every S-th stage: at least 4 each)
  S = (int)std::max<int64_t>(1, std::min<int64_t>(S, nst_min / 4));
  if (c.lat_ksplit > 0) S = (int)std::max<int64_t>(1, std::min<int64_t>(c.lat_ksplit, nst_min));
  // a power of two (the splits share the tile's cell passes), and with S > 1 every
  // GEMM workgroup of the launch resident at once (the splits of a tile wait for
  // each other): tiles x S within two workgroups per CU
  int p2 = 1;
  while (2 * p2 <= S) p2 *= 2;
  S = p2;
  while (S > 1 && tiles_sum * S > 2 * (int64_t)c.ncu) S /= 2;
  return S;
}

// w units: two per CU over the launch (equal shares of the F stream: with an
// uneven count the CUs holding one more unit set the stream's pace; two per CU
// keep twice the loads in flight: tools/probe_wloop.hip, B = 8: 25 vs 30 us),
// each GP's count by its F steps
// and at least ~8 steps each: a block's partials are summed by one unit, four
// partials per round trip (one GP at 128x128, N = 2048: 512 units 57.1 us per
// launch, 256 units 52.4, 128 units 52.7; tools/sweep_lat_b1.sh)
// ... and for a large batch about 512 steps each, up to eight units per CU (more
// loads queued: configs[4], 32 GPs at N = 8192, 2.86 ms per step with 512 units,
// 2.41 with 2048; the headline keeps 512: 384 and 448 were slower)
inline int64_t w_units(const Knobs& c, int64_t wsteps_sum) {
  int64_t wu_total = std::max<int64_t>(c.ncu / 2, wsteps_sum / 8);
  if (wu_total > 2 * c.ncu)
    wu_total = std::max<int64_t>(2 * c.ncu, std::min<int64_t>(8 * c.ncu, wsteps_sum / 512));
  if (c.lat_wu > 0) wu_total = c.lat_wu;
  return wu_total;
}
// the share of a GP of n0 rows: by its F steps, within [1, min(WU_MAX, its steps)]
inline int w_share(int64_t wu_total, int64_t wsteps_sum, int64_t n0) {
  const int64_t st = wsteps(n0);
  const int64_t u = (wu_total * st + wsteps_sum / 2) / wsteps_sum;
  return (int)std::max<int64_t>(1, std::min<int64_t>({u, (int64_t)WU_MAX, st}));
}

// The plan of a step over the n GPs g (each eligible for it: lat_eligible).
inline Plan plan(const Knobs& c, const Gp* g, int n) {
  Plan p{};
  p.take = true;
  p.ka = 8;
  p.ksplit = 1;
  for (int i = 0; i < n; ++i)
    if (g[i].k > 8) p.ka = 16;
  int64_t t2 = 0;
  for (int i = 0; i < n; ++i) t2 += tiles2(g[i].nx, g[i].ny, p.ka);
  p.g2 = second_launch(c, t2);
  int64_t nst_min = INT64_MAX;
  for (int i = 0; i < n; ++i) {
    p.tiles_sum += p.g2 ? tiles2(g[i].nx, g[i].ny, p.ka) : tiles(g[i].nx, g[i].ny, p.ka);
    // K stages of the axis rows (virtual rows add more)
    const int64_t nst = (g[i].sf ? 1 : 2) * (((int64_t)g[i].ny + KSTAGE - 1) / KSTAGE * KSTAGE / KSTAGE);
    nst_min = std::min(nst_min, nst);
  }
  if (!cheaper_than_vstream(g, n) && !c.lat_force) {
    p.take = false;
    return p;
  }
  p.ksplit = split_k(c, p.g2, p.tiles_sum, nst_min);
  for (int i = 0; i < n; ++i) p.wsteps_sum += wsteps(g[i].n0);
  p.wu_total = w_units(c, p.wsteps_sum);
  return p;
}

}  // namespace mfgp_lat_plan
