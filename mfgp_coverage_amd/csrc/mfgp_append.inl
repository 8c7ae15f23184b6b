// The bordered append's producers and finish (inc_*). Included by mfgp_kernels.hip.

// ---------------------------------------------------------------------------
// Incremental append. The reference refactors from
// scratch on every updt / updt_hifi (gp:257-268, gp:531-542 -> gp:254 / gp:529);
// the factor of the leading rows does not change, so appending rows [n0, N)
// (k = N - n0 <= KINC hifi rows) to a factor current for rows [0, n0) is the
// bordered Cholesky step
//   L21^T = L11^-1 K12,   L22 = chol(K22 - L21 L21^T),   z2 = L22^-1 (r2 - L21 z1)
// plus the new rows of the diagonal-block inverses. L21^T is a set of V columns:
// when every new point is a grid cell (the simulator samples only grid cells,
// sim:705 / sim:875) and V = L11^-1 psi^T is resident for rows < n0, column c of
// L21^T is V[:, cell(c)] -- psi(cell, X) and K(X, x_new) are the same numbers,
// same operation order (k_entry vs k_predict's psi). One launch (k_inc_stream,
// below): producer workgroups over 128-row chunks find the cells, gather the V
// columns into rows n0.. of A and sum their chunk's L21 L21^T, L21 z1 (MFMA); the
// last producer to arrive sums the partials and computes L22, z2 and the new
// Linv rows. Off the grid (or without a resident V) it solves L21^T itself by
// blocked forward substitution (one workgroup, f64 MFMA; slower, but general).
// ---------------------------------------------------------------------------
#ifndef MFGP_INC_WAVES
#define MFGP_INC_WAVES 4   // k_inc_stream waves per SIMD (occupancy; 5 measured 1-5 % slower)
#endif
constexpr int FCH = FUSED_CHUNK;           // rows of L21 per producer workgroup
constexpr int ISZ = KINC * KINC + KINC;    // partial sums per chunk: L21 L21^T | L21 z1
// iscr layout: [0] = 1 if the new points were found on the grid with V resident
// (k_append), [ISC0 + chunk * ISZ ...] = the producers' partials
constexpr int ISC0 = 1 + KINC;

// The L22 record the finish leaves for the cells (d.l22r): L22 [KINC][KINC] row-major | z2 [KINC].
// Entry e of it belongs to an append of k rows (the rest is staged as zeros): the lower
// triangle's first k rows, z2's first k entries.
__device__ __forceinline__ bool l22r_live(int e, int k) {
  return e < KINC * KINC ? (e / KINC < k && e % KINC <= e / KINC) : (e - KINC * KINC < k);
}
// The record into LDS by all NT threads; src(e, i): entry e, the i-th of this thread.
template <class Src>
__device__ __forceinline__ void l22r_stage(double* L22, int k, Src src) {
  for (int e = threadIdx.x, i = 0; e < KINC * KINC + KINC; e += NT, ++i) {
    const double v = src(e, i);
    L22[e] = l22r_live(e, k) ? v : 0.0;
  }
}
// Column c = threadIdx.x of L22^-1 (rows / columns >= k zero) into Li [KINC][KINC] by forward
// substitution, from the record staged in LDS (a barrier lies between).
__device__ __forceinline__ void l22inv_column(int k, const double* L22, double* Li) {
  if (threadIdx.x < KINC) {
    const int c = threadIdx.x;
    double x[KINC];
#pragma unroll
    for (int i = 0; i < KINC; ++i) {
      double t = (i == c) ? 1.0 : 0.0;
#pragma unroll
      for (int b = 0; b < i; ++b) t -= L22[i * KINC + b] * x[b];
      x[i] = (i < k && i >= c) ? t / L22[i * KINC + i] : 0.0;
      Li[i * KINC + c] = x[i];
    }
  }
}

// Coordinates / observation of training row `row`: rows landing in this launch
// ([N - k_new, N), device source) are read from the source itself.
__device__ __forceinline__ const double* row_pt(const GPDesc& d, int64_t row) {
  const int64_t at = d.N - d.k_new;
  if (row >= at && d.srcX) return d.srcX + 2 * (row - at);
  if (row >= at && d.rows_inline) return d.rows_xy + 2 * (row - at);
  return d.X + 2 * row;
}
__device__ __forceinline__ double row_obs(const GPDesc& d, int64_t row) {
  const int64_t at = d.N - d.k_new;
  if (row >= at && d.srcY) return d.srcY[row - at];
  if (row >= at && d.rows_inline) return d.rows_y[row - at];
  return d.y[row];
}

// Identity padding for the 64-row blocks [ablk, nbf) entered for the first time,
// columns [c_lo, c_hi) (the full predict reads whole blocks: padding rows must
// stay finite), and, with `linv`, their Linv blocks.
// Rows [skip_lo, skip_hi) are left out (the caller stores them itself).
template <bool XW = false>
__device__ void inc_init_blocks(const GPDesc& d, int64_t c_lo, int64_t c_hi, bool linv, int64_t skip_lo = 0,
                                int64_t skip_hi = 0) {
  const int64_t nbf = nblocks_factor(d.N);
  const int tid = threadIdx.x, nthr = blockDim.x;
  for (int64_t bb = d.ablk; bb < nbf; ++bb) {
    const int64_t c1 = c_hi < (bb + 1) * NB ? c_hi : (bb + 1) * NB;
    if (c1 > c_lo) {
      for (int64_t e = tid; e < (c1 - c_lo) * NB; e += nthr) {
        const int64_t col = c_lo + (e >> 6);
        const int64_t row = bb * NB + (e & 63);
        if (row < skip_lo || row >= skip_hi) stx<XW>(&d.A[col * d.ld + row], (col == row) ? 1.0 : 0.0);
      }
    }
    if (linv)
      for (int e = tid; e < TILE; e += nthr) d.Linv[bb * TILE + e] = ((e & 63) == (e >> 6)) ? 1.0 : 0.0;
  }
}

// The compact bordered row j, entry r, for the cell workgroups' MFMA A operand:
// fp64 V: L21[r][j] for r < k, z1[j] at r = k, zeros; fp32 V (VT = float, the
// rows stored as floats over the same area): L21[r][j] for r < k, z1[j] at
// r = ZROW (the f32 stream sums the mean out of that fixed row), zeros.
constexpr int ZROW = KINC - 1;
template <bool XW, class VT>
__device__ __forceinline__ void store_l21c(double* l21c, int64_t j, int r, int k, double a, double z) {
  if constexpr (sizeof(VT) == 8) {
    stx<XW>(&l21c[j * KINC + r], r < k ? a : (r == k ? z : 0.0));
  } else {
    float* p = reinterpret_cast<float*>(l21c) + j * KINC + r;
    const float v = (float)(r < k ? a : (r == ZROW ? z : 0.0));
    if constexpr (XW) __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else *p = v;
  }
}

// The resident V of this GP in the precision VT (fp64 d.V, fp32 d.Vf).
template <class VT>
__device__ __forceinline__ const VT* vres_ptr(const GPDesc& d) {
  if constexpr (sizeof(VT) == 8) return d.V;
  else return d.Vf;
}
// The column store of V (GPDesc::vcol) in the precision VT, or null.
template <class VT>
__device__ __forceinline__ const VT* vcol_ptr(const GPDesc& d) {
  return static_cast<const VT*>(d.vcol);
}
// The new rows [n0, n0 + k) of cell c into the column store: 8 k (fp32: 4 k) contiguous bytes,
// in 16-byte stores where n0 leaves them aligned (vcol_ld is a multiple of PRB); write-through
// (k_lat_gemm2's cells leave no dirty lines, as their other stores).
template <int KA, class VT>
__device__ __forceinline__ void vcol_store(const GPDesc& d, int64_t c, int64_t n0, int k, const double (&vn)[KA]) {
  VT* const p = const_cast<VT*>(vcol_ptr<VT>(d)) + c * d.vcol_ld + n0;
  constexpr int W = 16 / (int)sizeof(VT);   // elements per 16-byte store
  const bool al = (n0 & (W - 1)) == 0;
#pragma unroll
  for (int a = 0; a < KA; a += W) {
    if (al && a + W <= k) {
      if constexpr (sizeof(VT) == 8) {
        const dv2 v{vn[a], vn[a + 1]};
        st16_wt(p + a, v);
      } else {
        const f4 v{(float)vn[a], (float)vn[a + 1], (float)vn[a + 2], (float)vn[a + 3]};
        st16_wt(reinterpret_cast<double*>(p + a), __builtin_bit_cast(dv2, v));
      }
    } else {
#pragma unroll
      for (int b = 0; b < W; ++b)
        if (a + b < k) __hip_atomic_store(p + a + b, (VT)vn[a + b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

// Partial L21 L21^T and L21 z1 over rows [j_lo, j_hi) into red[w][ISZ] (one slot per
// wave). Lane (r, q) holds L21[r][j], j = 4s + q, eight 4-row steps in flight per
// wave. With `cell`, L21[r][.] is gathered from the V column of the grid cell and
// written to row n0 + r of A; otherwise it is read from there. VT: the precision
// of the resident V (an fp32 V's entries are widened: L21 is then the factor of K
// perturbed by their rounding, |dL21| <= 2^-24 |L21|).
template <int NW, bool XW, bool FROMV, class VT>
__device__ void inc_schur_partial(const GPDesc& d, const int* cell, int64_t j_lo, int64_t j_hi,
                                  double (*red)[ISZ]) {
  // descriptor fields in registers: the write-through stores below would make the
  // compiler reload them (and drain every load) before each store
  const int64_t n0 = d.n0, ld = d.ld;
  const int k = (int)(d.N - n0);
  double* const A = d.A;
  double* const l21c = d.l21c;
  const double* const zv = d.zv;
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 15, q = lane >> 4;
  d4 sacc = {0.0, 0.0, 0.0, 0.0}, uacc = {0.0, 0.0, 0.0, 0.0};
  constexpr int IU = 8;
  const int cr = (FROMV && r < k) ? cell[r] : 0;
  const VT* vsrc = FROMV ? vres_ptr<VT>(d) + (int64_t)(cr / PBM) * d.vld * PBM + (cr % PBM) : nullptr;
  const double* src = A + n0 + (r < k ? r : 0);
  const int64_t sstride = FROMV ? PBM : ld;
  const int64_t s_lo = j_lo >> 2, s_hi = (j_hi + 3) >> 2;   // j_lo is a multiple of 4
  for (int64_t s0 = s_lo + w; s0 < s_hi; s0 += NW * IU) {
    double a[IU], zz[IU];
#pragma unroll
    for (int u = 0; u < IU; ++u) {
      const int64_t j = 4 * (s0 + NW * u) + q;
      const bool ok = j < j_hi;
      const int64_t jj = ok ? j : j_lo;
      a[u] = FROMV ? (double)gp(vsrc)[jj * sstride] : ldx<XW>(src + jj * sstride);
      zz[u] = gp(zv)[jj];
    }
#pragma unroll
    for (int u = 0; u < IU; ++u) {
      const int64_t j = 4 * (s0 + NW * u) + q;
      const bool ok = j < j_hi;
      a[u] = (ok && r < k) ? a[u] : 0.0;
      zz[u] = ok ? zz[u] : 0.0;
      if (FROMV && r < k && ok) stx<XW>(&A[j * ld + n0 + r], a[u]);
      // compact rows for the cell tiles: L21 | z1 | zeros
      if (ok) store_l21c<XW, VT>(l21c, j, r, k, a[u], zz[u]);
      sacc = mfma(a[u], a[u], sacc);
      uacc = mfma(a[u], zz[u], uacc);
    }
  }
#pragma unroll
  for (int v = 0; v < 4; ++v) {
    red[w][(q + 4 * v) * KINC + r] = sacc[v];
    if (r == 0) red[w][KINC * KINC + q + 4 * v] = uacc[v];
  }
}

// cell[c] = first grid index equal to new point c (INT_MAX if none); all NTHR
// threads of the workgroup take part, SB grid loads in flight per thread.
template <int NTHR>
__device__ void find_cells(const GPDesc& d, const double* px, const double* py, int* cell) {
  const int tid = threadIdx.x;
  const GLOBAL dv2* g2 = reinterpret_cast<const GLOBAL dv2*>(gp(d.grid));
  constexpr int SB = 8;
  for (int64_t e0 = tid; e0 < d.M; e0 += (int64_t)NTHR * SB) {
    dv2 gxy[SB];
#pragma unroll
    for (int u = 0; u < SB; ++u) {
      const int64_t e = e0 + (int64_t)u * NTHR;
      gxy[u] = g2[e < d.M ? e : 0];
    }
#pragma unroll
    for (int u = 0; u < SB; ++u) {
      const int64_t e = e0 + (int64_t)u * NTHR;
      bool hit = false;
#pragma unroll
      for (int c = 0; c < KINC; ++c) hit = hit || (gxy[u].x == px[c] && gxy[u].y == py[c]);
      if (hit && e < d.M) {
#pragma unroll
        for (int c = 0; c < KINC; ++c)
          if (gxy[u].x == px[c] && gxy[u].y == py[c]) atomicMin(&cell[c], (int)e);
      }
    }
  }
}

// The rounded estimate of a coordinate's index on a lattice axis of n values from v0, `inv` = one
// over their spacing.
__device__ __forceinline__ int lat_round(double p, double v0, double inv, int n) {
  return (int)rint(fmin(fmax((p - v0) * inv, 0.0), (double)(n - 1)));
}

// Index of grid point (px, py) from the lattice structure: the rounded axis
// estimate and its neighbours, checked for exact equality (INT_MAX if none).
// The axes are strictly monotone, so an exact match is the only one.
__device__ int lattice_cell(const GPDesc& d, double px, double py) {
  const GridLattice& L = d.lat;
  if (L.nx <= 0 || !(px == px) || !(py == py)) return INT_MAX;
  const GLOBAL dv2* g2 = reinterpret_cast<const GLOBAL dv2*>(gp(d.grid));
  const int ix = lat_round(px, L.x0, L.xinv, L.nx), iy = lat_round(py, L.y0, L.yinv, L.ny);
  int64_t e[9];
#pragma unroll
  for (int t = 0; t < 9; ++t) {
    const int cx = ix + t / 3 - 1, cy = iy + t % 3 - 1;
    e[t] = (cx >= 0 && cx < L.nx && cy >= 0 && cy < L.ny) ? cx * L.sx + cy * L.sy : -1;
  }
  dv2 g[9];
#pragma unroll
  for (int t = 0; t < 9; ++t) g[t] = g2[e[t] >= 0 ? e[t] : 0];
  int hit = INT_MAX;
#pragma unroll
  for (int t = 0; t < 9; ++t)
    if (e[t] >= 0 && g[t].x == px && g[t].y == py) hit = (int)e[t];
  return hit;
}

// End of a gathering producer chunk: its compact rows (and L21 rows in A) are
// drained and announced in pflag[chunk] (the cell workgroups wait for these),
// then the chunk's partials (red, summed over the waves) are stored for the finish.
__device__ __forceinline__ bool inc_chunk_done(const GPDesc& d, int64_t chunk, double (*red)[ISZ]) {
  drain_stores();
  __syncthreads();
  if (threadIdx.x == 0) publish(d.pflag + chunk, d.epoch);
  FSTAMP(39);   // latest producer past its gather
  double* __restrict__ part = d.iscr + ISC0 + chunk * ISZ;
  for (int e = threadIdx.x; e < ISZ; e += NT) {
    double acc = 0.0;
#pragma unroll
    for (int w = 0; w < NT / 64; ++w) acc += red[w][e];
    stx<true>(part + e, acc);
  }
  return true;
}

// Fast path of a producer chunk (at most FUSED_CHUNK rows) on a lattice grid: each
// wave estimates the new points' cells itself (lane r < k: point r, the rounded
// axis estimate), gathers its rows of L21 from those V columns and checks the
// estimates against the grid coordinates in the same round trip. Every wave
// checks the same points, so the verdict is uniform; on a miss nothing has been
// stored and the caller takes the general path. Otherwise as inc_schur_partial
// (FROMV): L21 rows into A and the compact rows, partials into red, and the
// chunk's identity padding of newly entered blocks (rows [n0, N) excepted: they
// are the L21 stores, so no barrier orders the two).
// (Its row step and its write-out of the partials repeat inc_schur_partial's on purpose: one
// shared helper for either, by value or by reference, changed the code of all 16 k_inc_lat
// kernels and cost two of them two more spilled SGPRs)
template <class VT>
__device__ __forceinline__ bool inc_gather_fast(const GPDesc& d, int64_t j_lo, int64_t j_hi, double (*red)[ISZ]) {
  constexpr int NW = NT / 64, IU = 8;
  static_assert(4 * NW * IU >= FUSED_CHUNK, "one round of loads covers a chunk");
  const int64_t n0 = d.n0, ld = d.ld, N = d.N;
  const int k = (int)(N - n0);
  double* const A = d.A;
  double* const l21c = d.l21c;
  const double* const zv = d.zv;
  const GridLattice L = d.lat;
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 15, q = lane >> 4;
  const double* p = row_pt(d, n0 + (r < k ? r : 0));
  const double px = p[0], py = p[1];
  const int ix = lat_round(px, L.x0, L.xinv, L.nx), iy = lat_round(py, L.y0, L.yinv, L.ny);
  const int64_t cr = (px == px && py == py) ? ix * L.sx + iy * L.sy : 0;
  const dv2 g = reinterpret_cast<const GLOBAL dv2*>(gp(d.grid))[cr];
  // the cell's column: contiguous in the column store when it holds the n0 rows, else
  // PBM elements apart in V (a 128-byte line per row)
  const bool vc = d.lat_vcol != 0;
  const VT* src = vc ? vcol_ptr<VT>(d) + cr * d.vcol_ld : vres_ptr<VT>(d) + (cr / PBM) * d.vld * PBM + (cr % PBM);
  const int64_t sstr = vc ? 1 : PBM;
  double a[IU], zz[IU];
#pragma unroll
  for (int u = 0; u < IU; ++u) {
    const int64_t j = j_lo + 4 * (w + NW * u) + q;
    const int64_t jj = j < j_hi ? j : j_lo;
    a[u] = (double)gp(src)[jj * sstr];
    zz[u] = gp(zv)[jj];
  }
  const bool miss = r < k && !(g.x == px && g.y == py);
  if (__ballot(miss) != 0) return false;
  inc_init_blocks<true>(d, j_lo, j_hi, false, n0, N);
  d4 sacc = {0.0, 0.0, 0.0, 0.0}, uacc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int u = 0; u < IU; ++u) {
    const int64_t j = j_lo + 4 * (w + NW * u) + q;
    const bool ok = j < j_hi;
    a[u] = (ok && r < k) ? a[u] : 0.0;
    zz[u] = ok ? zz[u] : 0.0;
    if (r < k && ok) stx<true>(&A[j * ld + n0 + r], a[u]);
    if (ok) store_l21c<true, VT>(l21c, j, r, k, a[u], zz[u]);
    sacc = mfma(a[u], a[u], sacc);
    uacc = mfma(a[u], zz[u], uacc);
  }
#pragma unroll
  for (int v = 0; v < 4; ++v) {
    red[w][(q + 4 * v) * KINC + r] = sacc[v];
    if (r == 0) red[w][KINC * KINC + q + 4 * v] = uacc[v];
  }
  return true;
}

// One producer chunk: land device-resident new rows (chunk 0), find the new
// points' grid cells, gather their V columns into rows n0.. of A for rows
// [chunk * ch, +ch) and store the chunk's partials. Returns false when L21 is not
// a set of V columns (off the grid / no resident V): the finish solves for it.
// All NTHR threads take part; `cell` and `red` are in LDS.
// Test build only (tests/test_codeobj.py): MFGP_NOINLINE_PRODUCE outlines the
// producer, the shape that once stalled k_inc_stream for seconds; the test checks
// that such a build is caught (a call inside the kernel) and the product one is not.
#ifdef MFGP_NOINLINE_PRODUCE
#define MFGP_PRODUCE_INLINE __attribute__((noinline))
#else
#define MFGP_PRODUCE_INLINE __forceinline__
#endif
template <class VT>
__device__ MFGP_PRODUCE_INLINE bool inc_produce(const GPDesc& d, int64_t chunk, int64_t ch, int* cell,
                                                double (*red)[ISZ]) {
  constexpr int NTHR = NT;
  constexpr bool XW = true;
  const int64_t n0 = d.n0, N = d.N;
  const int k = (int)(N - n0);
  const int tid = threadIdx.x;
  const int64_t kn = d.k_new, at = N - kn;   // rows [at, N) arrive from srcX / srcY
  if (chunk == 0 && kn > 0 && (d.srcX || d.rows_inline)) {
    // consumers are later launches (this one reads the sources: row_pt / row_obs)
    for (int64_t e = tid; e < 3 * kn; e += NTHR) {
      if (e < 2 * kn) const_cast<double*>(d.X)[2 * at + e] = row_pt(d, at + e / 2)[e % 2];
      else const_cast<double*>(d.y)[at + e - 2 * kn] = row_obs(d, at + e - 2 * kn);
    }
  }
  const bool try_v = n0 > 0 && d.vres >= n0 && vres_ptr<VT>(d) != nullptr && d.M > 0;
  if (!try_v) {
    if (chunk == 0 && tid == 0) stx<XW>(d.iscr, 0.0);
    return false;
  }
  const int64_t j_lo = chunk * ch;
  const int64_t j_hi = j_lo + ch < n0 ? j_lo + ch : n0;
  if (d.lat.nx > 0 && j_lo < n0 && ch <= FUSED_CHUNK && inc_gather_fast<VT>(d, j_lo, j_hi, red)) {
    if (chunk == 0 && tid == 0) stx<XW>(d.iscr, 1.0);
    return inc_chunk_done(d, chunk, red);
  }
  if (tid < KINC) cell[tid] = INT_MAX;
  __syncthreads();
  // lattice grids: a few probes per point; otherwise (or for a point off the
  // lattice) every thread scans the grid
  if (tid < k) {
    const double* p = row_pt(d, n0 + tid);
    cell[tid] = lattice_cell(d, p[0], p[1]);
  }
  __syncthreads();
  bool found = true;
  for (int c = 0; c < k; ++c) found = found && cell[c] != INT_MAX;
  if (!found) {
    double px[KINC], py[KINC];
#pragma unroll
    for (int c = 0; c < KINC; ++c) {
      const double* p = row_pt(d, n0 + (c < k ? c : 0));
      px[c] = c < k ? p[0] : __builtin_nan("");
      py[c] = c < k ? p[1] : __builtin_nan("");
    }
    __syncthreads();
    if (tid < KINC) cell[tid] = INT_MAX;
    __syncthreads();
    find_cells<NTHR>(d, px, py, cell);
    __syncthreads();
  }
  if (XW) FSTAMP(38);   // latest producer with its cells
  bool use_v = true;
  for (int c = 0; c < k; ++c) use_v = use_v && cell[c] != INT_MAX;
  if (chunk == 0 && tid == 0) stx<XW>(d.iscr, use_v ? 1.0 : 0.0);
  if (!use_v || j_lo >= n0) return use_v;   // off the grid: the finish solves
  inc_init_blocks<XW>(d, j_lo, j_hi, false);   // this chunk's columns of newly entered blocks
  __syncthreads();
  inc_schur_partial<NTHR / 64, XW, true, VT>(d, cell, j_lo, j_hi, red);
  return inc_chunk_done(d, chunk, red);
}

// LDS of the finish step (doubles; 256 threads):
//   phase 1 (partials / L21 solve, L22):  red [0,1088) ssum [1088,1360) K22s [1360,1616) Ts [1616,2640)
//   phase 2 (new Linv rows):              Ln [0,1024) Ps [1024,2048) Lb [2048,3056)
//   both:                                 L22s [3056,3312)
// (26.5 KB: LDS would fit five workgroups of k_inc_stream per CU; its 128 VGPRs allow four)
constexpr int FIN_LDS = 3312;
constexpr int LBW = 16;   // Linv_OO columns staged per pass (63 rows x 16 = 1008 doubles)

// The finish of a bordered append for one GP (one workgroup of NT threads): sum
// the producers' partials (chunks of `ch` rows) or solve L21 (off the grid),
// L22 = chol(K22 - L21 L21^T), z2, then the new rows of the diagonal-block
// inverses. FUSED (inside k_inc_stream): signals `sync[1]` once L21 is in A (when
// this step solved it) and `sync[2]` once L22 / z2 are, with the hand-off
// accesses of ldx / stx.
template <bool FUSED, class VT>
__device__ __forceinline__ void inc_finish(const GPDesc& d, double* sm, int64_t ch) {
  const int64_t n0 = d.n0, N = d.N, ld = d.ld, NL = d.NL;
  const int k = (int)(N - n0);
  const Hyp& h = d.hf;
  double* __restrict__ A = d.A;
  const double* __restrict__ X = d.X;
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 15, q = lane >> 4;
  double(*red)[ISZ] = reinterpret_cast<double(*)[ISZ]>(sm);
  double* ssum = sm + 1088;
  double* K22s = sm + 1360;   // K22 (+ noise + jitter on the diagonal), row-major
  double* Ts = sm + 1616;     // T_I image [64][16]
  double* Ln = sm;            // new rows of L inside the current block, [i][m]
  double* Ps = sm + 1024;     // L_WO Linv_OO of the current block, [i][c]
  double* Lb = sm + 2048;     // Linv_OO columns [cb, cb + LBW), [m][c - cb]
  double* L22s = sm + 3056;   // L22, row-major
  const int64_t bb0 = n0 / NB;
  const int nO0 = (int)(n0 - bb0 * NB);   // old rows in block bb0
  STAMP(20);
  // write-through: with status_host the launch's last cell group reads it (drained
  // with the L22 record before sync[2])
  if (tid == 0) __hip_atomic_store(d.status, INT_MAX, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  {
    // one K22 entry per thread (gp:523-529 via k_entry)
    const int a = tid / KINC, b = tid % KINC;
    K22s[tid] = (a < k && b <= a) ? k_entry_pts(h, NL, n0 + a, row_pt(d, n0 + a), n0 + b, row_pt(d, n0 + b)) : 0.0;
  }
  const bool gathered = n0 > 0 && ldx<FUSED>(d.iscr) != 0.0;
  inc_init_blocks<FUSED>(d, gathered ? n0 : 0, nblocks_factor(N) * NB, true);
  __syncthreads();
  STAMP(21);
  if (gathered) {
    const int64_t nch = (n0 + ch - 1) / ch;
    for (int e = tid; e < ISZ; e += NT) {
      // chunk partials in a fixed order; eight loads in flight per thread
      double acc = 0.0;
      for (int64_t c0 = 0; c0 < nch; c0 += 8) {
        double t[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) t[u] = (c0 + u < nch) ? ldx<FUSED>(d.iscr + ISC0 + (c0 + u) * ISZ + e) : 0.0;
#pragma unroll
        for (int u = 0; u < 8; ++u) acc += t[u];
      }
      ssum[e] = acc;
    }
  } else {
    // L21^T = L11^-1 K12, left-looking: T_I = K12_I - sum_{J<I} L_IJ W_J;  W_I = Linv_II T_I
    const int64_t nb0 = (n0 + NB - 1) / NB;
    for (int64_t I = 0; I < nb0; ++I) {
      const int64_t i0 = I * NB + w * 16;   // this wave's 16 rows
      d4 acc;
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int64_t row = i0 + q + 4 * v;
        acc[v] = (row < n0 && r < k) ? k_entry_pts(h, NL, row, X + 2 * row, n0 + r, row_pt(d, n0 + r)) : 0.0;
      }
      for (int64_t J = 0; J < I; ++J) {
#pragma unroll 4
        for (int t = 0; t < NB / 4; ++t) {
          const int64_t kc = J * NB + 4 * t + q;
          const double a = A[kc * ld + i0 + r];                                // L[i0 + r][kc]
          const double b = (r < k) ? ldx<FUSED>(&A[kc * ld + n0 + r]) : 0.0;   // W[kc][r]
          acc = mfma(-a, b, acc);
        }
      }
#pragma unroll
      for (int v = 0; v < 4; ++v) Ts[(w * 16 + q + 4 * v) * KINC + r] = acc[v];
      __syncthreads();
      const double* __restrict__ Li = d.Linv + I * TILE;
      d4 o = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 4
      for (int t = 0; t < NB / 4; ++t) {
        const int m = 4 * t + q;
        o = mfma(Li[m * NB + w * 16 + r], Ts[m * KINC + r], o);
      }
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int64_t row = i0 + q + 4 * v;
        if (row < n0 && r < k) stx<FUSED>(&A[row * ld + n0 + r], o[v]);
      }
      if (FUSED) drain_stores();
      __syncthreads();   // W_I visible to every wave; Ts free
    }
    inc_schur_partial<NT / 64, FUSED, false, VT>(d, nullptr, 0, n0, red);
    if (FUSED) drain_stores();   // the compact rows, before sync[1]
    __syncthreads();
    for (int e = tid; e < ISZ; e += NT) ssum[e] = (red[0][e] + red[1][e]) + (red[2][e] + red[3][e]);
    if (FUSED && tid == 0) publish(d.sync + 1, d.epoch);   // L21 is in A
  }
  __syncthreads();
  STAMP(22);
  // L22 = chol(K22 - L21 L21^T) and z2, wave 0 (LAPACK dpotf2 order, as in
  // factor_invert_64; lane r holds row r, DPP row broadcasts)
  if (w == 0) {
    double dd[KINC];
#pragma unroll
    for (int c = 0; c < KINC; ++c) {
      double v = (r == c) ? 1.0 : 0.0;
      if (r < k && c < k) v = K22s[r * KINC + c] - ssum[r * KINC + c];
      dd[c] = v;
    }
    const double yr = (r < k) ? row_obs(d, n0 + r) : 0.0;
    double rdiag = 1.0;
    int fail = INT_MAX;
#pragma unroll
    for (int j = 0; j < KINC; ++j) {
      double p = bcast16(dd[j], j);
      const bool pad = j >= k;
      const bool bad = !pad && !(p > 0.0);
      fail = bad ? min(fail, (int)(n0 + j + 1)) : fail;
      p = (pad || bad) ? 1.0 : p;
      const double rs = rsqrt(p);
      const double l = (r > j) ? dd[j] * rs : (r == j ? p * rs : 0.0);
      rdiag = (r == j) ? rs : rdiag;
      dd[j] = l;
      const double lu = (r > j) ? l : 0.0;
#pragma unroll
      for (int kk = j + 1; kk < KINC; ++kk) dd[kk] -= lu * bcast16(l, kk);
    }
    // z2 = L22^-1 (r2 - L21 z1), r2 = y - m_H (new rows are hifi; gp:133 / gp:421)
    double x = 0.0;
    if (r < k) x = (yr - h.meanH) - ssum[KINC * KINC + r];
#pragma unroll
    for (int j = 0; j < KINC; ++j) {
      if (r == j) x *= rdiag;
      const double zj = bcast16(x, j);
      if (r > j) x -= dd[j] * zj;
    }
    if (lane < k) {
#pragma unroll
      for (int c = 0; c < KINC; ++c) {
        L22s[lane * KINC + c] = (c <= lane) ? dd[c] : 0.0;
        if (c <= lane) stx<FUSED>(&A[(n0 + c) * ld + n0 + lane], dd[c]);
        // the record the cell workgroups read (no line of it is read before sync[2])
        stx<FUSED>(&d.l22r[lane * KINC + c], (c <= lane) ? dd[c] : 0.0);
      }
      stx<FUSED>(&d.zv[n0 + lane], x);
      stx<FUSED>(&d.l22r[KINC * KINC + lane], x);
    }
    if (fail != INT_MAX && lane == 0) atomicMin(d.status, fail);
    // the step's positive-definiteness verdict as soon as it is known (a mapped host
    // word: the eager append returns here while the posterior is still computed)
    if (FUSED && d.pd_host && lane == 0) __hip_atomic_store(d.pd_host, fail, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    if (FUSED) {
      drain_stores();
      if (lane == 0) publish(d.sync + 2, d.epoch);   // L22 and z2 are in A / zv
      WTRACE(3);
      if (FUSED) FSTAMP(32);
    }
  }
  __syncthreads();
  STAMP(23);
  // new rows' old-column part of block bb0 (L21 entries, in A)
  for (int e = tid; e < k * NB; e += NT) {
    const int i = e >> 6, m = e & 63;
    if (m < nO0) Ln[i * NB + m] = ldx<FUSED>(&A[(bb0 * NB + m) * ld + n0 + i]);
  }
  __syncthreads();
  STAMP(24);
  // new rows of the diagonal-block inverses. In block bb, with old rows O and new
  // rows W (a triangular inverse's rows do not depend on later rows):
  //   Linv_WO = -L_WW^-1 (L_WO Linv_OO),   Linv_WW = L_WW^-1
  // thread c: column c of the new rows, by forward substitution over the <= 16 new rows
  for (int64_t bb = bb0; bb * NB < N; ++bb) {
    double* __restrict__ Li = d.Linv + bb * TILE;
    const int64_t r0 = n0 > bb * NB ? n0 : bb * NB;
    const int64_t r1 = N < (bb + 1) * NB ? N : (bb + 1) * NB;
    const int nO = (int)(r0 - bb * NB), nW = (int)(r1 - r0);
    const int a0 = (int)(r0 - n0);   // first new row of this block, as a row of L22
    // L22 part of the new rows (columns n0.. of this block)
    for (int e = tid; e < nW * NB; e += NT) {
      const int i = e >> 6, m = e & 63;
      const int64_t col = bb * NB + m;
      if (col >= n0) {
        const int b = (int)(col - n0);
        Ln[i * NB + m] = (b <= a0 + i) ? L22s[(a0 + i) * KINC + b] : 0.0;
      } else if (bb != bb0) {
        Ln[i * NB + m] = ldx<FUSED>(&A[col * ld + r0 + i]);
      }
    }
    __syncthreads();
    // P = L_WO Linv_OO: element (i, c) per thread, Linv_OO lower triangular (its
    // upper part is stored as zeros), so the sum runs over all old rows m;
    // Linv_OO is staged through LDS LBW columns at a time
    for (int cb = 0; cb < nO; cb += LBW) {
      for (int e = tid; e < nO * LBW; e += NT) {
        const int c = e / nO, m = e - c * nO;   // consecutive threads: consecutive rows of one column
        Lb[m * LBW + c] = (cb + c < NB) ? Li[(cb + c) * NB + m] : 0.0;
      }
      __syncthreads();
      for (int e = tid; e < nW * LBW; e += NT) {
        const int i = e / LBW, c = e % LBW;
        double p0 = 0.0, p1 = 0.0, p2 = 0.0, p3 = 0.0;
        int m = 0;
        for (; m + 4 <= nO; m += 4) {
          p0 += Ln[i * NB + m] * Lb[m * LBW + c];
          p1 += Ln[i * NB + m + 1] * Lb[(m + 1) * LBW + c];
          p2 += Ln[i * NB + m + 2] * Lb[(m + 2) * LBW + c];
          p3 += Ln[i * NB + m + 3] * Lb[(m + 3) * LBW + c];
        }
        for (; m < nO; ++m) p0 += Ln[i * NB + m] * Lb[m * LBW + c];
        Ps[i * NB + cb + c] = (p0 + p1) + (p2 + p3);
      }
      __syncthreads();
    }
    if (tid < NB) {
      const int c = tid;
      double xs[KINC];
#pragma unroll
      for (int i = 0; i < KINC; ++i) {
        xs[i] = 0.0;
        if (i < nW) {
          double t = (c < nO) ? -Ps[i * NB + c] : ((c == nO + i) ? 1.0 : 0.0);
#pragma unroll
          for (int i2 = 0; i2 < i; ++i2) t -= Ln[i * NB + nO + i2] * xs[i2];
          xs[i] = t / Ln[i * NB + nO + i];
          Li[c * NB + nO + i] = xs[i];
        }
      }
    }
    __syncthreads();
  }
  STAMP(25);
}

// Producer role `role` < nprod of a fused append launch (k_inc_stream, k_inc_lat):
// gather its chunk of L21 and the partials, drain, count the arrival (sync[0]);
// the last one signals sync[1] (L21 complete, when gathered), runs inc_finish
// (which signals sync[1] itself when it solves L21, then sync[2]) and resets
// sync[0] for the next launch.
// `cell` [KINC] and `last` are LDS words of the caller's.
template <class VT>
__device__ __forceinline__ void inc_producer_role(const GPDesc& d, int64_t role, double* sm, int* cell,
                                                  unsigned& last) {
  const int64_t np = d.nprod;
  if (role == 0) FSTAMP(30);
  __builtin_amdgcn_s_setprio(3);   // producers and the finish before the cell streams
  const bool gathered = inc_produce<VT>(d, role, FCH, cell, reinterpret_cast<double(*)[ISZ]>(sm));
  FSTAMP(40);   // latest producer done storing (before the drain)
  drain_stores();
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned old = __hip_atomic_fetch_add(d.sync, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    last = (old == (unsigned)(np - 1)) ? 1u : 0u;
    if (last) {
      __hip_atomic_store(d.sync, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (gathered) publish(d.sync + 1, d.epoch);   // every chunk of L21 is in A
    }
  }
  FSTAMP(31);   // latest producer arrival
  __syncthreads();
  WTRACE(1);
  if (last) inc_finish<true, VT>(d, sm, FCH);
  if (last) WTRACE(2);   // the hand-off accesses: tiles may stream concurrently
  WTRACE(4);
}
