// The one-pass predict (ws_*, wf_*, vstream_wg*, k_vstream) and the fused append + predict
// launch (k_inc_stream*). Included by mfgp_kernels.hip.

// ---------------------------------------------------------------------------
// Incremental predict: V is resident for rows < n0 and the factor has k = N - n0
// <= KINC new rows (k = 0: nothing appended since the last predict).
//   T      = psi_new^T - L21 V_old      (16 x n0 by n0 x 32 per wave, f64 MFMA)
//   V_new  = L22^-1 T                   -> rows [n0, N) of the resident V
//   var    = k** - colsum(V o V),  mu = m + V^T z   over all N rows
// V_old is read once: the kernel is HBM-bound. A workgroup covers 128 cells (two
// 64-cell V tiles) and each of its waves owns 32 cells over ALL n0 rows, so the
// stream needs no LDS and no barrier and a workgroup streams once per launch:
// at the headline size every cell workgroup is resident at once (one round, no
// tile-to-tile transitions, whose startup and epilogue round trips under full
// load left half the chip idle in the middle of the launch).
// Lane (r, q) of a wave: cells 2r, 2r + 1 of the wave's 32 (one 16-byte load per
// row), rows 4s + q of row step s; MFMA B operand = the cells' values, A operand =
// L21c[row][r] (rows r < k of L21, z1 at r = k, zeros above), so MFMA output row
// a is T (seeded with -psi_new) and row k is V_old^T z1. A ring of WS_S stages of
// WS_U row steps keeps WS_S - 1 stages of loads in flight while one is consumed.
// ---------------------------------------------------------------------------
constexpr int WS_CELLS = 32;            // cells per wave
constexpr int WS_WG = 4 * WS_CELLS;     // cells per workgroup (two V tiles; ntiles_wg)
// LDS of a cell workgroup (doubles): L22 (row-major) | z2 | new rows' (x, y) |
// cells' (x, y) | the row splits' partials (R = 4: 3 slots of 12 x 64)
constexpr int VS_LDS = KINC * KINC + KINC + 2 * KINC + 2 * WS_WG + 3 * 12 * 64;
static_assert(WS_WG == 2 * PBM, "a cell workgroup is two V tiles");
#ifndef MFGP_WS_U
#define MFGP_WS_U 2
#endif
#ifndef MFGP_WS_S
#define MFGP_WS_S 4
#endif
constexpr int WS_U = MFGP_WS_U, WS_S = MFGP_WS_S;
static_assert(WS_S >= 2, "a ring of at least two stages");

// psi of grid cell (gx, gy) against new training row g at (tx, ty): SF k, MF
// [rho k_L | rho^2 k_L + k_H] by the row's fidelity (gp:426-429), in the
// reference's operation order (as k_predict's psi)
__device__ __forceinline__ double psi_new(const Hyp& h, int64_t NL, int64_t g, double gx, double gy, double tx,
                                          double ty) {
#pragma clang fp contract(off)
  const double cLx = div_(gx, h.lL), cLy = div_(gy, h.lL);
  const double tLx = div_(tx, h.lL), tLy = div_(ty, h.lL);
  if (h.kind == 0) return se_scaled(cLx, cLy, tLx, tLy, h.sL);
  if (g < NL) return h.rho * se_scaled(cLx, cLy, tLx, tLy, h.sL);
  return h.rho2 * se_scaled(cLx, cLy, tLx, tLy, h.sL) +
         se_scaled(div_(gx, h.lH), div_(gy, h.lH), div_(tx, h.lH), div_(ty, h.lH), h.sH);
}

// MODE 0: k = 0 (no MFMA; V^T z by VALU). MODE 1: MFMA on L21 read from A (row
// stride ld, lanes r >= k masked), V^T z by VALU (k = KINC, or the compact rows
// are not for these rows). MODE 2: MFMA on the compact rows, V^T z1 = row k.
// Row steps per stage by mode: the rare modes carry z (and mask) registers and
// take one step per stage to stay inside the occupancy's register budget.
template <int MODE>
constexpr int ws_u() { return MODE == 2 ? WS_U : (MODE == 1 ? 1 : 2); }
template <int MODE>
constexpr int ws_s() { return MODE == 2 ? WS_S : (MODE == 1 ? 4 : 3); }

// A ring stage carries its shape: U row steps per stage, S stages in the ring, and the
// accumulator type its rows are summed into.
template <int MODE>
struct WsStage {
  static constexpr int U = ws_u<MODE>(), S = ws_s<MODE>();
  using Acc = d4;
  dv2 v[U];
  double a[U], z[U];
};

template <int MODE>
struct WsSrc {
  const GLOBAL dv2* vb;       // this lane's cells, row 0
  const GLOBAL double* ab;    // A operand, row 0 (MODE >= 1)
  int64_t astride;
  const GLOBAL double* zb;    // z, row 0 (MODE <= 1)
  int64_t n0;                 // end of this wave's row range
  int64_t j_lo;               // start of it (a multiple of 8)
};

// Rows j0 + 4u (u < WS_U) of this lane; GUARD clamps rows >= n0 to row 0.
template <bool GUARD, int MODE>
__device__ __forceinline__ void stage_load(WsStage<MODE>& s, const WsSrc<MODE>& src, int64_t j0) {
#pragma unroll
  for (int u = 0; u < ws_u<MODE>(); ++u) {
    const int64_t j = j0 + 4 * u;
    const int64_t jj = (!GUARD || j < src.n0) ? j : 0;   // clamped, loads stay unconditional
    // V is read once per update and is far larger than the Infinity Cache
    s.v[u] = __builtin_nontemporal_load(src.vb + jj * (PBM / 2));
    if (MODE >= 1) s.a[u] = src.ab[jj * src.astride];
    if (MODE <= 1) s.z[u] = src.zb[jj];
  }
}

// MODE 0 (the re-predict of an unchanged model) sums each cell's rows in four
// classes, (row mod 64) / 16, combined as ((0 + 1) + (2 + 3)) at the end: the
// order of k_predict's four waves, so a second predict() returns the same bits.
template <bool GUARD, int MODE>
__device__ __forceinline__ void stage_use(WsStage<MODE>& s, int64_t j0, int64_t n0, bool arow, d4* acc, double* vs,
                                          double* ms) {
  const int cls = MODE == 0 ? (int)((j0 & 63) >> 4) : 0;   // uniform: j0 = 4t + q
#pragma unroll
  for (int u = 0; u < ws_u<MODE>(); ++u) {
    if (GUARD && j0 + 4 * u >= n0) {
      s.v[u] = dv2{0.0, 0.0};
      s.a[u] = 0.0;
      s.z[u] = 0.0;
    }
    if (MODE == 0) {
#pragma unroll
      for (int c = 0; c < 4; ++c)
        if (c == cls) {   // explicit fma: k_predict's contracted a += x * y
          vs[2 * c] = __builtin_fma(s.v[u].x, s.v[u].x, vs[2 * c]);
          vs[2 * c + 1] = __builtin_fma(s.v[u].y, s.v[u].y, vs[2 * c + 1]);
          ms[2 * c] = __builtin_fma(s.v[u].x, s.z[u], ms[2 * c]);
          ms[2 * c + 1] = __builtin_fma(s.v[u].y, s.z[u], ms[2 * c + 1]);
        }
      continue;
    }
    vs[0] += s.v[u].x * s.v[u].x;
    vs[1] += s.v[u].y * s.v[u].y;
    if (MODE <= 1) {
      ms[0] += s.z[u] * s.v[u].x;
      ms[1] += s.z[u] * s.v[u].y;
    }
    if (MODE >= 1) {
      const double a = (MODE == 1 && !arow) ? 0.0 : s.a[u];
      acc[0] = mfma(a, s.v[u].x, acc[0]);
      acc[1] = mfma(a, s.v[u].y, acc[1]);
    }
  }
}

// The epilogue's L22 record, fetched during the stream: the sync[2] flag is read
// halfway (fused launches), the record itself at three quarters if the flag was
// up, so the epilogue skips both round trips (the finish publishes long before).
struct WsPrefetch {
  const unsigned* flag;   // null: nothing to prefetch
  unsigned epoch;
  const double* rec;      // KINC * KINC + KINC doubles
  unsigned fval;
  double r0, r1;          // rec[tid], rec[tid + NT] (tid + NT < record size)
  bool have;
};

__device__ __forceinline__ void ws_prefetch(WsPrefetch& pf, int64_t t, int64_t T) {
  if (!pf.flag) return;
  const int tid = threadIdx.x;
  if (t == T / 2) pf.fval = __hip_atomic_load(pf.flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (t == (3 * T) / 4) {
    pf.have = pf.fval == pf.epoch;
    if (pf.have) {
      // plain loads: no line of the record is read in this launch before sync[2]
      pf.r0 = pf.rec[tid];
      pf.r1 = tid + NT < KINC * KINC + KINC ? pf.rec[tid + NT] : 0.0;
    }
  }
}

// First row of a source's range, and what ends a pass of the ring: nothing for the fp64 stages
// (the fp32 ones: below, with their stage).
template <int MODE>
__device__ __forceinline__ int64_t src_j_lo(const WsSrc<MODE>& src) { return src.j_lo; }
template <int MODE>
__device__ __forceinline__ void stage_pass_end(const WsStage<MODE>*, d4*, double*, int) {}

// The row range [j_lo, n0) of this lane's cells through a software ring of Stage::S stages: full
// stages pipelined, the ragged last stage guarded. Stage is WsStage (fp64 V) or WfStage (fp32 V);
// stage_load / stage_use / stage_pass_end are overloaded on it. q0: this lane's row residue.
template <class Stage, class Src>
__device__ __forceinline__ void ring_stream(const Src& src, int q0, bool arow, typename Stage::Acc* acc, double* vs,
                                            double* ms, WsPrefetch& pf) {
  constexpr int64_t RS = 4 * Stage::U;   // rows per stage
  constexpr int SS = Stage::S;           // stages in the ring
  const int64_t n0 = src.n0, j_lo = src_j_lo(src);
  const int64_t q = j_lo + q0;           // this lane's first row
  const int64_t T = (n0 - j_lo) / RS;    // full stages
  Stage st[SS];
#pragma unroll
  for (int s = 0; s < SS - 1; ++s)
    if (s < T) stage_load<false>(st[s], src, s * RS + q);
  int64_t t = 0;
  // steady state (sched_barrier keeps each stage's loads ahead of the use after it)
  for (; t + 2 * SS - 1 <= T; t += SS) {
    // the workgroups of a CU stream at unequal rates (the memory pipe favours the
    // oldest waves: 195 / 250 / 309 / 339 us for the four slots of a CU, measured),
    // so priority falls as a wave advances and the waves of a CU finish closer
    // together (3 stays with the producers and the finish, which the streams wait for)
    if (t >= (2 * T) / 3) __builtin_amdgcn_s_setprio(0);
    else if (t >= T / 3) __builtin_amdgcn_s_setprio(1);
    else __builtin_amdgcn_s_setprio(2);
#pragma unroll
    for (int s = 0; s < SS; ++s) ws_prefetch(pf, t + s, T);
#pragma unroll
    for (int s = 0; s < SS; ++s) {
      stage_load<false>(st[(s + SS - 1) % SS], src, (t + s + SS - 1) * RS + q);
      __builtin_amdgcn_sched_barrier(0);
      stage_use<false>(st[s], (t + s) * RS + q, n0, arow, acc, vs, ms);
      __builtin_amdgcn_sched_barrier(0);
    }
    stage_pass_end(st, acc, ms, q0);
  }
  // drain: fewer than 2 SS - 1 full stages left
#pragma unroll
  for (int s = 0; s < 2 * SS - 2; ++s) {
    if (t + s >= T) break;
    if (t + s + SS - 1 < T) stage_load<false>(st[(s + SS - 1) % SS], src, (t + s + SS - 1) * RS + q);
    stage_use<false>(st[s % SS], (t + s) * RS + q, n0, arow, acc, vs, ms);
  }
  if (j_lo + T * RS < n0) {
    const int64_t j0 = T * RS + q;
    stage_load<true>(st[0], src, j0);
    stage_use<true>(st[0], j0, n0, arow, acc, vs, ms);
  }
  stage_pass_end(st, acc, ms, q0);
}

// Arrival of one wave's cell group (slot) of the launch, with its (max, first
// argmax) of var when the fused var max / argmax is asked for. The last group of
// the launch to arrive reduces the partials and, with status_host, copies the
// GP's status word into the mapped host word (every status write of the launch
// -- the finish's, a wait's timeout -- is drained before its group counts in).
// Write-through partials, a drain and a relaxed counter: no fence (a release
// fence writes the whole L2 back).
// The drain is the calling wave's own (s_waitcnt vmcnt(0)): an arrival says nothing
// of other waves' stores. The stream kernels call this behind their group's stores.
// k_lat_gemm2 without status_host calls it on a wave that stores nothing, ahead of
// its tile's cell stores: there the (max, argmax) and the count are all an arrival
// carries, and the outputs are visible at the launch's end; with status_host it
// keeps the order of the stream kernels (lat_gemm2, mfgp_lattice.inl).
__device__ void var_argmax_group(const GPDesc& d, double bv, int64_t bi, int64_t slot, int64_t nslots) {
  const int lane = threadIdx.x & 63;
  const bool red = d.vmax || d.vargmax;
  unsigned* cnt = reinterpret_cast<unsigned*>(d.tred);   // tred = [counter | (max, argmax) per group]
  double* part = d.tred + 1;
  if (red) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) argmax_pair(bv, bi, __shfl_xor(bv, off), __shfl_xor(bi, off));
  }
  unsigned old = 0;
  if (lane == 0) {
    if (red) {
      __hip_atomic_store(part + 2 * slot, bv, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(part + 2 * slot + 1, (double)bi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    old = __hip_atomic_fetch_add(cnt, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  old = __shfl(old, 0);
  if (old != (unsigned)(nslots - 1)) return;
  if (red) {
    bv = -__builtin_inf();
    bi = INT64_MAX;
    for (int64_t t = lane; t < nslots; t += 64)
      argmax_pair(bv, bi, __hip_atomic_load(part + 2 * t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT),
                  (int64_t)__hip_atomic_load(part + 2 * t + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) argmax_pair(bv, bi, __shfl_xor(bv, off), __shfl_xor(bi, off));
  }
  if (lane == 0) {
    if (d.vmax) *d.vmax = bv;
    if (d.vargmax) *d.vargmax = bi;
    if (d.status_host) *d.status_host = __hip_atomic_load(d.status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(cnt, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// Value of register `v` of lane `src` (all lanes take part).
__device__ __forceinline__ double lane_get(double v, int src) { return __shfl(v, src); }

// ---- what the fp64 and the fp32 cell workgroups share (vstream_wg, vstream_wg_f32) ----

// L22 | z2 of an unfused launch (written by an earlier launch) into LDS: the record of
// the append that wrote the compact rows, else A / zv.
__device__ __forceinline__ void vs_record_unfused(const GPDesc& d, int64_t n0, int64_t ld, int k, double* L22) {
  for (int e = threadIdx.x; e < KINC * KINC + KINC; e += NT) {
    double v = 0.0;
    if (e < KINC * KINC) {
      const int ra = e / KINC, cb = e % KINC;
      if (ra < k && cb <= ra) v = d.l21c_ok ? d.l22r[e] : d.A[(n0 + cb) * ld + n0 + ra];
    } else if (e - KINC * KINC < k) {
      v = d.l21c_ok ? d.l22r[e] : d.zv[n0 + e - KINC * KINC];
    }
    L22[e] = v;
  }
}

// The prefetch of a fused launch's record during the stream (`on`), or none.
__device__ __forceinline__ WsPrefetch vs_prefetch(const GPDesc& d, bool on) {
  return WsPrefetch{on ? d.sync + 2 : nullptr, d.epoch, d.l22r, 0u, 0.0, 0.0, false};
}

// L22 / z2 of a fused launch (sync[2]) into LDS: from the stream's prefetch if every wave
// had it, else now. Ends with the workgroup's barrier (fused or not).
template <bool FUSED>
__device__ __forceinline__ void vs_record_arrives(const GPDesc& d, int k, bool mma, const WsPrefetch& pf, double* L22) {
  const bool pre = (FUSED && mma) ? __syncthreads_and(pf.have) != 0 : false;
  if (pre) l22r_stage(L22, k, [&](int, int i) { return i == 0 ? pf.r0 : pf.r1; });
  if (FUSED && mma && !pre) {
    // the workgroup's waves end their streams together
    wait_flag(d, d.sync + 2, d.epoch);
    // plain loads: no line of the record is read in this launch before sync[2]
    // (an L2 miss for the first workgroup of an XCD, hits for the others)
    l22r_stage(L22, k, [&](int e, int) { return d.l22r[e]; });
  }
  __syncthreads();
}

// The new rows of V of this lane's cell, vn = L22^-1 T by forward substitution, and their
// terms of var and mu. t_of(a): the accumulators' entry of row a for this cell, fetched
// from the lane that holds it (-(psi_new - L21 V_old)).
template <class TOf>
__device__ __forceinline__ void vs_solve(int k, const double* L22, TOf t_of, double (&vn)[KINC], double& vsum,
                                         double& msum) {
#pragma unroll
  for (int a = 0; a < KINC; ++a) {
    vn[a] = 0.0;
    if (a < k) {
      double t = -t_of(a);   // psi_new - L21 V_old
#pragma unroll
      for (int b = 0; b < a; ++b) t -= L22[a * KINC + b] * vn[b];
      vn[a] = t / L22[a * KINC + a];
      vsum += vn[a] * vn[a];
      msum += vn[a] * L22[KINC * KINC + a];
    }
  }
}

// This lane's cell c out (`valid`: it has one): mu, var and the resident posterior; then the
// arrival of its wave's group of CELLS cells from cg (`arrive`: the group counts).
template <int CELLS>
__device__ __forceinline__ void vs_output(const GPDesc& d, int64_t cg, int64_t c, bool valid, bool arrive,
                                          double vsum, double msum) {
  const Hyp& h = d.hp;
  const double vc = h.kss - vsum;
  if (valid) {
    d.mu[c] = msum + h.meanH;
    d.var[c] = vc;
    if (d.rmu) {
      d.rmu[c] = msum + h.meanH;
      d.rvar[c] = vc;
    }
  }
  if ((d.vmax || d.vargmax || d.status_host) && arrive)
    var_argmax_group(d, valid ? vc : -__builtin_inf(), valid ? c : INT64_MAX, cg / CELLS, (d.M + CELLS - 1) / CELLS);
}

// One workgroup of the one-pass predict: 128 / R cells, R = d.rsplit row splits.
// Wave w owns cell group w % (4 / R) (32 cells) over row split w / (4 / R); with
// R > 1 (small batches, so that the chip still holds ~4 workgroups per CU) the
// splits' partial sums meet in LDS, added in split order. FUSED (inside
// k_inc_stream): the compact rows are read once sync[1] is signalled, L22 / z2
// once sync[2] is.
template <bool FUSED>
__device__ __forceinline__ void vstream_wg(const GPDesc& d, int64_t wgt, double* sm) {
  const int64_t M = d.M;
  const int64_t n0 = d.n0, N = d.N, ld = d.ld;
  const int k = (int)(N - n0);
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 15, q = lane >> 4;
  const int R = d.rsplit;                   // 1, 2 or 4 (uniform)
  const int ncg = 4 / R;                    // cell groups per workgroup
  const int cpw = WS_CELLS * ncg;           // cells per workgroup
  const int si = w / ncg;                   // this wave's row split
  const int64_t cg = wgt * cpw + WS_CELLS * (w % ncg);   // first grid cell of this wave
  const int64_t vt = cg / PBM;              // its V tile
  const int cw = (int)(cg % PBM);           // and first cell inside it
  const bool live = cg < M;                 // a ragged last workgroup may hold empty groups
  double* __restrict__ Vt = d.V + vt * d.vld * PBM;
  const Hyp& h = d.hp;
  double* L22 = sm;                          // L22 (row-major) | z2
  double* Xn = sm + KINC * KINC + KINC;      // new rows' (x, y)
  double* Gc = Xn + 2 * KINC;                // the workgroup's cells' (x, y)
  const int64_t c0 = cg + 2 * r;             // this lane's cells c0, c0 + 1
  d4 acc[2];
  acc[0] = d4{0.0, 0.0, 0.0, 0.0};
  acc[1] = d4{0.0, 0.0, 0.0, 0.0};
  double vs[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, ms[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  const bool mma = k > 0;
  const bool zrow = mma && k < KINC && d.l21c_ok;
  if (!FUSED && mma) vs_record_unfused(d, n0, ld, k, L22);
  if (mma) {
    // the psi_new inputs through LDS (one 16-byte load per thread: the producers'
    // round trips at the start of the launch run beside this traffic)
    if (tid < cpw) {
      const int64_t cc = wgt * cpw + tid < M ? wgt * cpw + tid : M - 1;
      reinterpret_cast<dv2*>(Gc)[tid] = *reinterpret_cast<const GLOBAL dv2*>(gp(d.grid) + 2 * cc);
    } else if (tid >= NT - KINC) {
      const int a = tid - (NT - KINC);
      const double* p = row_pt(d, n0 + (a < k ? a : 0));
      Xn[2 * a] = p[0];
      Xn[2 * a + 1] = p[1];
    }
    __syncthreads();
  }
  if (live && mma && si == 0) {
    {
      // T = psi_new^T - L21 V_old: the accumulators start at -psi_new (MFMA output
      // row q + 4v of lane (r, q), cells c0 + x), so the epilogue has no exps left
      const int e0 = (int)(c0 - wgt * cpw);
      const double g0x = Gc[2 * e0], g0y = Gc[2 * e0 + 1], g1x = Gc[2 * e0 + 2], g1y = Gc[2 * e0 + 3];
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int a = q + 4 * v;
        if (a < k) {
          const double tx = Xn[2 * a], ty = Xn[2 * a + 1];
          acc[0][v] = -psi_new(h, d.NL, n0 + a, g0x, g0y, tx, ty);
          acc[1][v] = -psi_new(h, d.NL, n0 + a, g1x, g1y, tx, ty);
        }
      }
    }
  }
  if (FUSED && mma) wait_l21_from(d, 0);   // the compact rows of this append (all waves)
  WsPrefetch pf = vs_prefetch(d, FUSED && mma);
  if (FUSED) WTRACE(1);
  // this wave's rows: split si of [0, n0) at multiples of 8 rows; a re-predict
  // (k = 0) streams all rows in split 0 (the exact summation order of k_predict)
  int64_t j_lo = 0, j_hi = n0;
  if (R > 1) {
    if (!mma) {
      j_hi = si == 0 ? n0 : 0;
    } else {
      j_lo = (si * n0 / R) & ~(int64_t)7;
      j_hi = si == R - 1 ? n0 : ((si + 1) * n0 / R) & ~(int64_t)7;
    }
  }
  if (live && j_hi > j_lo) {
    const GLOBAL dv2* vb = reinterpret_cast<const GLOBAL dv2*>(gp(Vt)) + (cw >> 1) + r;
    if (zrow) {
      const WsSrc<2> src{vb, gp(d.l21c) + r, KINC, nullptr, j_hi, j_lo};
      ring_stream<WsStage<2>>(src, q, true, acc, vs, ms, pf);
    } else if (mma) {
      const WsSrc<1> src{vb, gp(d.A) + n0 + (r < k ? r : 0), ld, gp(d.zv), j_hi, j_lo};
      ring_stream<WsStage<1>>(src, q, r < k, acc, vs, ms, pf);
    } else {
      const WsSrc<0> src{vb, nullptr, 0, gp(d.zv), j_hi, j_lo};
      ring_stream<WsStage<0>>(src, q, false, acc, vs, ms, pf);
    }
  }
  if (R > 1 && mma) {
    // the row splits' partials meet in LDS (lane-for-lane, before the lane
    // reductions), added to split 0's in split order
    double* part = Gc + 2 * WS_WG;   // [(R - 1) * ncg slots][12][64]
    if (si > 0) {
      double* pp = part + ((si - 1) * ncg + w % ncg) * 12 * 64 + lane;
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        pp[v * 64] = acc[0][v];
        pp[(4 + v) * 64] = acc[1][v];
      }
      pp[8 * 64] = vs[0];
      pp[9 * 64] = vs[1];
      pp[10 * 64] = ms[0];
      pp[11 * 64] = ms[1];
    }
    __syncthreads();
    if (si == 0) {
      for (int sj = 1; sj < R; ++sj) {
        const double* pp = part + ((sj - 1) * ncg + w % ncg) * 12 * 64 + lane;
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          acc[0][v] += pp[v * 64];
          acc[1][v] += pp[(4 + v) * 64];
        }
        vs[0] += pp[8 * 64];
        vs[1] += pp[9 * 64];
        ms[0] += pp[10 * 64];
        ms[1] += pp[11 * 64];
      }
    }
  }
  // colsums over the lanes' row residues q (and, for k = 0, the four row classes)
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    if (e >= 2 && mma) break;
    vs[e] += __shfl_xor(vs[e], 16);
    vs[e] += __shfl_xor(vs[e], 32);
    ms[e] += __shfl_xor(ms[e], 16);
    ms[e] += __shfl_xor(ms[e], 32);
  }
  if (!mma) {
#pragma unroll
    for (int x = 0; x < 2; ++x) {
      vs[x] = (vs[x] + vs[2 + x]) + (vs[4 + x] + vs[6 + x]);
      ms[x] = (ms[x] + ms[2 + x]) + (ms[4 + x] + ms[6 + x]);
    }
  }
  if (FUSED) WTRACE(2);
  vs_record_arrives<FUSED>(d, k, mma, pf, L22);
  if (FUSED) WTRACE(3);
  // epilogue: lane (r, x) with x = q < 2 finishes cell c0 + x. Row a of T for that
  // cell sits in acc[x][a / 4] of lane (r, a % 4).
  const int x = q & 1;
  const int64_t c = c0 + x;
  double vsum = x ? vs[1] : vs[0];
  double msum = x ? ms[1] : ms[0];
  if (mma) {
    if (zrow) {
      const double m0 = lane_get(acc[0][k / 4], r + 16 * (k % 4));
      const double m1 = lane_get(acc[1][k / 4], r + 16 * (k % 4));
      msum += x ? m1 : m0;
    }
    double vn[KINC];
    vs_solve(k, L22, [&](int a) {
      const double t0 = lane_get(acc[0][a / 4], r + 16 * (a % 4));
      const double t1 = lane_get(acc[1][a / 4], r + 16 * (a % 4));
      return x ? t1 : t0;
    }, vn, vsum, msum);
    if (live && si == 0 && q < 2 && c < M) {
#pragma unroll
      for (int a = 0; a < KINC; ++a)
        if (a < k) {
          gp(Vt)[(n0 + a) * PBM + cw + 2 * r + x] = vn[a];
        }
    }
  }
  vs_output<WS_CELLS>(d, cg, c, live && si == 0 && q < 2 && c < M, cg < M && si == 0, vsum, msum);
  if (FUSED) WTRACE(4);
}

// ---------------------------------------------------------------------------
// One-pass predict over an fp32 V (MFGP_F32 models, BASELINE configs[4]): the
// same algorithm as vstream_wg, with V stored in fp32 -- half the bytes of the
// HBM-bound stream. Everything but V stays fp64: the factor, z, L21 (widened
// from the V gather), L22, the epilogue's solve for V_new, and both reductions
// (var = k** - colsum(V o V) and mu = m + V^T z accumulate in f64).
// Lane (r, q) of a wave: cells 4r .. 4r + 3 of the wave's 64 (one 64-cell V
// tile; one 16-byte load per row), rows 4s + q of row step s. T = psi_new^T -
// L21 V_old on the exact f32 MFMA (v_mfma_f32_16x16x4_f32), one per cell slot
// x: A = the compact rows (fp32: L21 rows 0..k-1, z1 in row ZROW), B = the
// slot's V entries; output lane (r, g) register v = row 4g + v, cell 4r + x.
// Row ZROW (lanes g = 3, register 3) is V_old^T z1: it is added into f64 and
// cleared once per pass of the stage ring, so no f32 sum runs over more than 32
// rows. T itself accumulates in f32 over all n0 rows (its error is divided by
// L22 >= sqrt(noise_H) in V_new). No row splits: 256 cells per workgroup.
// ---------------------------------------------------------------------------
constexpr int WF_CELLS = 64;            // cells per wave (one V tile)
constexpr int WF_WG = 4 * WF_CELLS;     // cells per workgroup (ntiles_wg(M, 1, 1))
constexpr int WF_LDS = KINC * KINC + KINC + 2 * KINC + 2 * WF_WG;
static_assert(WF_LDS <= FIN_LDS, "one LDS image serves every role");
static_assert(WF_WG == NT, "one thread per cell of the workgroup stages the psi inputs");
#ifndef MFGP_WF_S
#define MFGP_WF_S 4
#endif

// MODE as ws_*: 0 = k = 0 (VALU mean over z), 1 = A operand from A (widened
// to f32 per load; VALU mean), 2 = compact rows (mean from row ZROW).
template <int MODE>
constexpr int wf_u() { return 2; }
template <int MODE>
constexpr int wf_s() { return MODE == 2 ? MFGP_WF_S : 3; }

template <int MODE>
struct WfStage {
  static constexpr int U = wf_u<MODE>(), S = wf_s<MODE>();
  using Acc = f4;
  f4 v[U];
  float a[U];
  double z[U];
};

struct WfSrc {
  const GLOBAL f4* vb;        // this lane's cells, row 0
  const GLOBAL float* af;     // MODE 2: compact rows, this lane's entry of row 0
  const GLOBAL double* ad;    // MODE 1: A, row n0 + r of column 0
  int64_t astride;
  const GLOBAL double* zb;    // z, row 0 (MODE <= 1)
  int64_t n0;
};
__device__ __forceinline__ int64_t src_j_lo(const WfSrc&) { return 0; }   // no row splits

template <bool GUARD, int MODE>
__device__ __forceinline__ void stage_load(WfStage<MODE>& s, const WfSrc& src, int64_t j0) {
#pragma unroll
  for (int u = 0; u < wf_u<MODE>(); ++u) {
    const int64_t j = j0 + 4 * u;
    const int64_t jj = (!GUARD || j < src.n0) ? j : 0;
    s.v[u] = __builtin_nontemporal_load(src.vb + jj * (PBM / 4));
    if (MODE == 2) s.a[u] = src.af[jj * KINC];
    if (MODE == 1) s.a[u] = (float)src.ad[jj * src.astride];
    if (MODE <= 1) s.z[u] = src.zb[jj];
  }
}

template <bool GUARD, int MODE>
__device__ __forceinline__ void stage_use(WfStage<MODE>& s, int64_t j0, int64_t n0, bool arow, f4* acc, double* vs,
                                          double* ms) {
#pragma unroll
  for (int u = 0; u < wf_u<MODE>(); ++u) {
    if (GUARD && j0 + 4 * u >= n0) {
      s.v[u] = f4{0.f, 0.f, 0.f, 0.f};
      s.a[u] = 0.f;
      s.z[u] = 0.0;
    }
    double vx[4];
#pragma unroll
    for (int x = 0; x < 4; ++x) {
      vx[x] = (double)s.v[u][x];
      vs[x] = __builtin_fma(vx[x], vx[x], vs[x]);
      if (MODE <= 1) ms[x] = __builtin_fma(vx[x], s.z[u], ms[x]);
    }
    if (MODE >= 1) {
      const float a = (MODE == 1 && !arow) ? 0.f : s.a[u];
#pragma unroll
      for (int x = 0; x < 4; ++x) acc[x] = mfma(a, s.v[u][x], acc[x]);
    }
  }
}

// Row ZROW of the accumulators (lanes g = 3, register 3) into the f64 mean sums.
__device__ __forceinline__ void wf_flush_zrow(f4* acc, double* ms, bool zl) {
  static_assert(ZROW == 15, "row 15 = lane group 3, register 3");
#pragma unroll
  for (int x = 0; x < 4; ++x) {
    const float t = acc[x][3];
    ms[x] += zl ? (double)t : 0.0;
    acc[x][3] = zl ? 0.f : t;
  }
}

// End of a ring pass (and of the stream): the compact rows' mean row goes to f64.
template <int MODE>
__device__ __forceinline__ void stage_pass_end(const WfStage<MODE>*, f4* acc, double* ms, int q0) {
  if (MODE == 2) wf_flush_zrow(acc, ms, q0 == 3);
}

// Pick element x of a per-slot quadruple (x uniform per lane).
__device__ __forceinline__ double pick4(double a0, double a1, double a2, double a3, int x) {
  return x == 0 ? a0 : (x == 1 ? a1 : (x == 2 ? a2 : a3));
}

// One workgroup of the fp32 one-pass predict: 256 cells, wave w owns cells
// [wgt * 256 + 64 w, +64) over all n0 rows. FUSED as vstream_wg.
template <bool FUSED>
__device__ __forceinline__ void vstream_wg_f32(const GPDesc& d, int64_t wgt, double* sm) {
  const int64_t M = d.M;
  const int64_t n0 = d.n0, N = d.N, ld = d.ld;
  const int k = (int)(N - n0);
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 15, q = lane >> 4;
  const int64_t cg = wgt * WF_WG + WF_CELLS * w;   // first grid cell of this wave = its V tile's
  const bool live = cg < M;
  float* __restrict__ Vt = d.Vf + (cg / PBM) * d.vld * PBM;
  const Hyp& h = d.hp;
  double* L22 = sm;                          // L22 (row-major) | z2
  double* Xn = sm + KINC * KINC + KINC;      // new rows' (x, y)
  double* Gc = Xn + 2 * KINC;                // the workgroup's cells' (x, y)
  f4 acc[4];
#pragma unroll
  for (int x = 0; x < 4; ++x) acc[x] = f4{0.f, 0.f, 0.f, 0.f};
  double vs[4] = {0.0, 0.0, 0.0, 0.0}, ms[4] = {0.0, 0.0, 0.0, 0.0};
  const bool mma = k > 0;
  const bool zrow = mma && k < KINC && d.l21c_ok;
  if (!FUSED && mma) vs_record_unfused(d, n0, ld, k, L22);
  if (mma) {
    {
      const int64_t cc = wgt * WF_WG + tid < M ? wgt * WF_WG + tid : M - 1;
      reinterpret_cast<dv2*>(Gc)[tid] = *reinterpret_cast<const GLOBAL dv2*>(gp(d.grid) + 2 * cc);
    }
    if (tid < KINC) {
      const double* p = row_pt(d, n0 + (tid < k ? tid : 0));
      Xn[2 * tid] = p[0];
      Xn[2 * tid + 1] = p[1];
    }
    __syncthreads();
  }
  if (live && mma) {
    // the accumulators start at -psi_new (row 4q + v of cell 4r + x), in f32
    const int e0 = WF_CELLS * w + 4 * r;
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int a = 4 * q + v;
      if (a < k) {
        const double tx = Xn[2 * a], ty = Xn[2 * a + 1];
#pragma unroll
        for (int x = 0; x < 4; ++x)
          acc[x][v] = (float)(-psi_new(h, d.NL, n0 + a, Gc[2 * (e0 + x)], Gc[2 * (e0 + x) + 1], tx, ty));
      }
    }
  }
  if (FUSED && mma) wait_l21_from(d, 0);
  WsPrefetch pf = vs_prefetch(d, FUSED && mma);
  if (live && n0 > 0) {
    const GLOBAL f4* vb = reinterpret_cast<const GLOBAL f4*>(gp(Vt)) + r;
    if (zrow) {
      const WfSrc src{vb, reinterpret_cast<const GLOBAL float*>(gp(d.l21c)) + r, nullptr, 0, nullptr, n0};
      ring_stream<WfStage<2>>(src, q, true, acc, vs, ms, pf);
    } else if (mma) {
      const WfSrc src{vb, nullptr, gp(d.A) + n0 + (r < k ? r : 0), ld, gp(d.zv), n0};
      ring_stream<WfStage<1>>(src, q, r < k, acc, vs, ms, pf);
    } else {
      const WfSrc src{vb, nullptr, nullptr, 0, gp(d.zv), n0};
      ring_stream<WfStage<0>>(src, q, false, acc, vs, ms, pf);
    }
  }
  // colsums over the lanes' row residues q
#pragma unroll
  for (int x = 0; x < 4; ++x) {
    vs[x] += __shfl_xor(vs[x], 16);
    vs[x] += __shfl_xor(vs[x], 32);
    ms[x] += __shfl_xor(ms[x], 16);
    ms[x] += __shfl_xor(ms[x], 32);
  }
  vs_record_arrives<FUSED>(d, k, mma, pf, L22);
  // epilogue: lane (r, q) finishes cell cg + 4r + q (slot x = q). Row a of T for
  // slot x sits in acc[x][a % 4] of lane (r, a / 4).
  const int x = q;
  const int64_t c = cg + 4 * r + x;
  double vsum = pick4(vs[0], vs[1], vs[2], vs[3], x);
  double msum = pick4(ms[0], ms[1], ms[2], ms[3], x);
  if (mma) {
    double vn[KINC];
    vs_solve(k, L22, [&](int a) {
      const int src = r + 16 * (a / 4);
      const double t0 = (double)__shfl(acc[0][a % 4], src);
      const double t1 = (double)__shfl(acc[1][a % 4], src);
      const double t2 = (double)__shfl(acc[2][a % 4], src);
      const double t3 = (double)__shfl(acc[3][a % 4], src);
      return pick4(t0, t1, t2, t3, x);
    }, vn, vsum, msum);
    if (live && c < M) {
#pragma unroll
      for (int a = 0; a < KINC; ++a)
        if (a < k) gp(Vt)[(n0 + a) * PBM + 4 * r + x] = (float)vn[a];
    }
  }
  vs_output<WF_CELLS>(d, cg, c, live && c < M, live, vsum, msum);
}

// Cells per one-pass-predict workgroup of descriptor d.
template <class VT>
__device__ __forceinline__ int64_t wg_cells(const GPDesc& d) {
  if constexpr (sizeof(VT) == 8) return WS_WG / d.rsplit;
  else return WF_WG;
}

template <class VT>
__global__ __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(MFGP_INC_WAVES, MFGP_INC_WAVES))) void k_vstream(
    const GPDesc* __restrict__ descs) {
  const GPDesc& d = descs[blockIdx.y];
  if ((int64_t)blockIdx.x * wg_cells<VT>(d) >= d.M) return;
  if (d.gate && *d.gate == 0) return;
  __shared__ double sm[VS_LDS > WF_LDS ? VS_LDS : WF_LDS];
  if constexpr (sizeof(VT) == 8) vstream_wg<false>(d, blockIdx.x, sm);
  else vstream_wg_f32<false>(d, blockIdx.x, sm);
}

// ---------------------------------------------------------------------------
// The bordered append (k_inc_stream). Grid (GPs, roles); per GP, roles < nprod
// are producers (inc_produce on FCH-row chunks of L21):
//   producers : gather L21 into A and their partials, drain, count arrivals
//               (sync[0]); the last one signals sync[1] (L21 complete, when
//               gathered), runs inc_finish (signals sync[1] itself when it
//               solves L21, then sync[2] once L22 / z2 are stored) and resets
//               sync[0] for the next launch.
// With d.tiles the same launch also runs the one-pass predict: roles >= nprod
// stream the 128-cell workgroups (vstream_wg<true>), waiting for sync[1] before
// the first L21 load and for sync[2] before the L22 solve of the epilogue. x = GP,
// so the linear dispatch order is every GP's producer 0, then producer 1, ...,
// then the cell workgroups round-robin over the GPs: producers are dispatched
// before any workgroup that waits for them and are therefore resident (no
// deadlock); the waits are bounded anyway. The flags hold the launch's epoch
// (host counter, never 0), so they need no reset. Without tiles nothing waits.
// Four workgroups per CU (128 VGPRs; 26.5 KB of LDS): at the headline size
// (8 GPs: 128 producers + 1024 cell workgroups) 1024 are resident at once and
// the last 128 cell workgroups take the producers' slots as they finish (9-15 us).
// ---------------------------------------------------------------------------
template <class VT>
__device__ __forceinline__ void inc_stream_wg(const GPDesc& d) {
  const int k = (int)(d.N - d.n0);
  if (k <= 0 || k > KINC) return;   // the host guarantees 0 < k <= KINC
  if (d.gate && *d.gate == 0) return;
  static_assert(VS_LDS <= FIN_LDS, "one LDS image serves every role");
  __shared__ double sm[FIN_LDS];
  WTRACE(0);
  const int64_t np = d.nprod, role = blockIdx.y;
  if (role >= np) {
    const int64_t wgt = role - np;
    if (d.tiles && wgt * wg_cells<VT>(d) < d.M) {
      if constexpr (sizeof(VT) == 8) vstream_wg<true>(d, wgt, sm);
      else vstream_wg_f32<true>(d, wgt, sm);
    }
    return;
  }
  __shared__ int cell[KINC];
  __shared__ unsigned last;
  inc_producer_role<VT>(d, role, sm, cell, last);
}

template <class VT>
__global__ __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(MFGP_INC_WAVES, MFGP_INC_WAVES))) void k_inc_stream(
    const GPDesc* __restrict__ descs) {
  inc_stream_wg<VT>(descs[blockIdx.x]);
}

// One GP, descriptor by value (kernarg segment: no upload copy before the launch).
template <class VT>
__global__ __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(MFGP_INC_WAVES, MFGP_INC_WAVES))) void k_inc_stream1(
    const GPDesc d) {
  inc_stream_wg<VT>(d);
}

// A batch of <= DESC_ARG_MAX GPs with the descriptors as the kernel argument
// (k_inc_lat_arg's reason: no per-step upload through the copy engine); the
// kernarg segment is indexed directly, a dynamic index into the by-value
// parameter would copy it to scratch.
template <class VT>
__global__ __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(MFGP_INC_WAVES, MFGP_INC_WAVES))) void k_inc_stream_arg(
    const DescArg a) {
  (void)a;
  const GPDesc* descs = (const GPDesc*)__builtin_amdgcn_kernarg_segment_ptr();
  inc_stream_wg<VT>(descs[blockIdx.x]);
}
