// Device-side helpers shared by the HIP translation units of libmfgp_hip.so
// (mfgp_kernels.hip, mfgp_nlml.hip, mfgp_cov.hip, mfgp_ivr.hip, mfgp_look.hip): f64 MFMA tile products,
// LDS tile staging, the SE kernel in the reference's operation order
// (gaussian_process.py:66-79), the K entries of gp:253-254 / gp:523-529, the 64x64
// diagonal-block factor and inverse, and the steps of the left-looking forward
// substitution that k_predict and the look-ahead kernels share.
#pragma once
#include <climits>
#include <hip/hip_runtime.h>

#include "mfgp_internal.h"

namespace mfgp {

typedef double d4 __attribute__((ext_vector_type(4)));
typedef double dv2 __attribute__((ext_vector_type(2)));
typedef float fv2 __attribute__((ext_vector_type(2)));
typedef float f4 __attribute__((ext_vector_type(4)));

// Generic -> global address space, so loads/stores through descriptor pointers
// are emitted as global_* (vmcnt only) instead of flat_* (vmcnt + lgkmcnt).
#define GLOBAL __attribute__((address_space(1)))
template <class T>
__device__ __forceinline__ GLOBAL T* gp(T* p) {
  return (GLOBAL T*)p;
}
template <class T>
__device__ __forceinline__ const GLOBAL T* gp(const T* p) {
  return (const GLOBAL T*)p;
}

__device__ __forceinline__ int swz(int k, int i) { return k * NB + (i ^ ((k & 1) << 4)); }

__device__ __forceinline__ d4 mfma(double a, double b, d4 c) {
  return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
}
// v_mfma_f64_4x4x4_4b_f64: four independent 4 x 4 x 4 blocks; lane l = 16 k + 4 blk + r
// holds A_blk[r][k] and B_blk[k][r], and C lane 16 i + 4 blk + j holds C_blk[i][j]
// (tools/probe_mfma4.hip, one-hot products); 1.64x the multiply-adds per cycle of
// the 16x16x4 form on gfx950
__device__ __forceinline__ double mfma4(double a, double b, double c) {
  return __builtin_amdgcn_mfma_f64_4x4x4f64(a, b, c, 0, 0, 0);
}
// exact f32 (v_mfma_f32_16x16x4_f32 = an fmaf chain). A/B lane maps as the f64
// form; C/D: lane (r, g) register v holds row 4g + v, column r (the f64 form:
// row g + 4v).
__device__ __forceinline__ f4 mfma(float a, float b, f4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// Per-wave 32x32 accumulator = 2x2 MFMA tiles of 16x16.
struct Acc {
  d4 c[2][2];
};

__device__ __forceinline__ void acc_zero(Acc& a) {
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int n = 0; n < 2; ++n) a.c[m][n] = d4{0.0, 0.0, 0.0, 0.0};
}

// acc (+/-)= A[64x64] * B[64x64] restricted to this wave's 32x32 output block.
// As[swz(k,i)] = A[i][k], Bs[swz(k,j)] = B[k][j].
template <bool NEG>
__device__ __forceinline__ void tile_mma(const double* __restrict__ As, const double* __restrict__ Bs,
                                         Acc& acc, int wm, int wn, int lane) {
  const int r = lane & 15, q = lane >> 4;
#pragma unroll 4
  for (int k0 = 0; k0 < NB; k0 += 4) {
    const int k = k0 + q;
    double a0 = As[swz(k, wm * 32 + r)];
    double a1 = As[swz(k, wm * 32 + 16 + r)];
    const double b0 = Bs[swz(k, wn * 32 + r)];
    const double b1 = Bs[swz(k, wn * 32 + 16 + r)];
    if (NEG) {
      a0 = -a0;
      a1 = -a1;
    }
    acc.c[0][0] = mfma(a0, b0, acc.c[0][0]);
    acc.c[0][1] = mfma(a0, b1, acc.c[0][1]);
    acc.c[1][0] = mfma(a1, b0, acc.c[1][0]);
    acc.c[1][1] = mfma(a1, b1, acc.c[1][1]);
  }
}

// Ts[swz(k,i)] = G[(c0+k)*ld + r0 + i], k,i in [0,64): a column-major 64x64 tile,
// each source column becoming one k-row. 16-byte loads, coalesced along i.
__device__ __forceinline__ void load_tile_cm(double* __restrict__ Ts, const double* __restrict__ G,
                                             int64_t ld, int64_t r0, int64_t c0, int tid) {
#pragma unroll
  for (int p = 0; p < 8; ++p) {
    const int k = p * 8 + (tid >> 5);
    const int i = (tid & 31) * 2;
    const dv2 v = *reinterpret_cast<const GLOBAL dv2*>(gp(G) + (c0 + k) * ld + r0 + i);
    *reinterpret_cast<dv2*>(Ts + swz(k, i)) = v;
  }
}

// Register staging of a column-major 64x64 tile (issue-early / write-late):
// fetch_tile_cm issues the 8 16-byte global loads per thread; store_tile writes
// them to the swizzled k-major LDS image once the buffer is free.
struct Stage {
  dv2 v[8];
};

__device__ __forceinline__ void fetch_tile_cm(Stage& st, const double* __restrict__ G, int64_t ld, int64_t r0,
                                              int64_t c0, int tid) {
#pragma unroll
  for (int p = 0; p < 8; ++p) {
    const int k = p * 8 + (tid >> 5);
    const int i = (tid & 31) * 2;
    st.v[p] = *reinterpret_cast<const GLOBAL dv2*>(gp(G) + (c0 + k) * ld + r0 + i);
  }
}

__device__ __forceinline__ void store_tile(double* __restrict__ Ts, const Stage& st, int tid) {
#pragma unroll
  for (int p = 0; p < 8; ++p) {
    const int k = p * 8 + (tid >> 5);
    const int i = (tid & 31) * 2;
    *reinterpret_cast<dv2*>(Ts + swz(k, i)) = st.v[p];
  }
}

// stage one 64x64 operand tile through registers (8 16-byte loads per thread)
struct TileRegs {
  dv2 v[8];
};
__device__ __forceinline__ void tile_fetch(TileRegs& t, const double* __restrict__ G, int64_t ld, int tid) {
#pragma unroll
  for (int p = 0; p < 8; ++p) t.v[p] = *reinterpret_cast<const GLOBAL dv2*>(gp(G) + (p * 8 + (tid >> 5)) * ld + (tid & 31) * 2);
}
// the tile's memory rows become k-rows: Ts[swz(k, i)] = G[k * ld + i]
__device__ __forceinline__ void tile_put_k(double* __restrict__ Ts, const TileRegs& t, int tid) {
#pragma unroll
  for (int p = 0; p < 8; ++p) {
    const int k = p * 8 + (tid >> 5), i = (tid & 31) * 2;
    *reinterpret_cast<dv2*>(Ts + swz(k, i)) = t.v[p];
  }
}
// transposed: Ts[swz(k, i)] = G[i * ld + k]
__device__ __forceinline__ void tile_put_t(double* __restrict__ Ts, const TileRegs& t, int tid) {
#pragma unroll
  for (int p = 0; p < 8; ++p) {
    const int i = p * 8 + (tid >> 5), k = (tid & 31) * 2;
    Ts[swz(k, i)] = t.v[p].x;
    Ts[swz(k + 1, i)] = t.v[p].y;
  }
}

constexpr int PW = 128;                  // row width of the predict L image (= PRB)
typedef __attribute__((address_space(3))) void* lds_vptr;

__device__ __forceinline__ int swzp(int k, int i) { return k * PW + (i ^ ((k & 1) << 4)); }

// DMA kn rows of 128 doubles into a swizzled [kn][128] LDS image:
// dst[swzp(k, i)] = G[(c0 + k) * ld + r0 + i]. One wave-instruction moves one 1 KB row.
__device__ __forceinline__ void dma_rows128(double* dst, const double* __restrict__ G, int64_t ld, int64_t r0,
                                            int64_t c0, int kn, int w, int lane) {
  for (int k = w; k < kn; k += PNT / 64) {
    const int i = (2 * lane) ^ ((k & 1) << 4);
    const double* src = G + (c0 + k) * ld + r0 + i;
    __builtin_amdgcn_global_load_lds((const GLOBAL void*)src, (lds_vptr)(dst + k * PW), 16, 0, 0);
  }
}

// DMA kn rows of 64 doubles into a swizzled [kn][64] LDS image:
// dst[swz(k, i)] = G[(c0 + k) * ld + r0 + i]. One wave-instruction moves two rows.
__device__ __forceinline__ void dma_rows64(double* dst, const double* __restrict__ G, int64_t ld, int64_t r0,
                                           int64_t c0, int kn, int w, int lane) {
  for (int p = w; p < kn / 2; p += PNT / 64) {
    const int k = 2 * p + (lane >> 5);
    const int i = ((lane & 31) * 2) ^ ((k & 1) << 4);
    const double* src = G + (c0 + k) * ld + r0 + i;
    __builtin_amdgcn_global_load_lds((const GLOBAL void*)src, (lds_vptr)(dst + 2 * p * NB), 16, 0, 0);
  }
}

__device__ __forceinline__ void vm_wait_all() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

// (max, first position) of two candidates: the larger value, the lower index on ties
// (np.argmax's rule)
__device__ __forceinline__ void argmax_pair(double& bv, int64_t& bi, double ov, int64_t oi) {
  if (ov > bv || (ov == bv && oi < bi)) {
    bv = ov;
    bi = oi;
  }
}

// C/D element (mt, nt, v) of this lane <-> tile (row, col).
__device__ __forceinline__ int acc_row(int wm, int mt, int q, int v) { return wm * 32 + mt * 16 + q + 4 * v; }
__device__ __forceinline__ int acc_col(int wn, int nt, int r) { return wn * 32 + nt * 16 + r; }

// ---------------------------------------------------------------------------
// Squared-exponential kernel, gaussian_process.py:66-79, in the reference's
// operation order: scale each coordinate by the length scale (a division),
// subtract, square, sum over D = 2, exp(-0.5 * .), times the output scale.
// No FMA contraction, so the rounding matches NumPy's elementwise ops.
// ---------------------------------------------------------------------------
__device__ __forceinline__ double se_scaled(double ax, double ay, double bx, double by, double s) {
#pragma clang fp contract(off)
  const double dx = ax - bx;
  const double dy = ay - by;
  const double d2 = dx * dx + dy * dy;
  return s * exp(-0.5 * d2);
}

__device__ __forceinline__ double div_(double a, double b) {
#pragma clang fp contract(off)
  return a / b;
}

// K entry (i, j), both < N, jitter and noise included (gp:253-254 / gp:523-529).
// pi / pj: the rows' coordinates (x, y).
__device__ __forceinline__ double k_entry_pts(const Hyp& h, int64_t NL, int64_t gi, const double* pi, int64_t gj,
                                              const double* pj) {
#pragma clang fp contract(off)
  const double xi = pi[0], yi = pi[1];
  const double xj = pj[0], yj = pj[1];
  const double kl = se_scaled(div_(xi, h.lL), div_(yi, h.lL), div_(xj, h.lL), div_(yj, h.lL), h.sL);
  double v;
  if (h.kind == 0) {
    v = kl;
    if (gi == gj) v = (v + h.noiseL) + h.jitter;
  } else {
    const bool li = gi < NL, lj = gj < NL;
    if (li && lj) {
      v = kl;                                            // K_LL (gp:523)
      if (gi == gj) v = (v + h.noiseL) + h.jitter;
    } else if (li != lj) {
      v = h.rho * kl;                                    // K_LH (gp:524)
    } else {
      const double kh = se_scaled(div_(xi, h.lH), div_(yi, h.lH), div_(xj, h.lH), div_(yj, h.lH), h.sH);
      v = h.rho2 * kl + kh;                              // K_HH (gp:525-526)
      if (gi == gj) v = (v + h.noiseH) + h.jitter;
    }
  }
  return v;
}
__device__ __forceinline__ double k_entry(const Hyp& h, const double* __restrict__ X, int64_t NL, int64_t gi,
                                          int64_t gj) {
  return k_entry_pts(h, NL, gi, X + 2 * gi, gj, X + 2 * gj);
}

__device__ __forceinline__ void tri_index(int64_t t, int& I, int& J) {
  int i = (int)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
  while ((int64_t)(i + 1) * (i + 2) / 2 <= t) ++i;
  while ((int64_t)i * (i + 1) / 2 > t) --i;
  I = i;
  J = (int)(t - (int64_t)i * (i + 1) / 2);
}

// ---------------------------------------------------------------------------
// Cholesky and explicit inverse of a 64x64 diagonal block (k_potrf_diag, whose
// header in mfgp_kernels.hip describes the algorithm, and k_look_border).
// ---------------------------------------------------------------------------
constexpr int SP = NB + 1;   // padded row stride of the row-major LDS tiles
constexpr int DB = 16;       // sub-block
constexpr int DP = DB + 1;

__device__ __forceinline__ double readlane_d(double v, int l) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), l);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
  return __hiloint2double(hi, lo);
}

// Broadcast lane k of each 16-lane DPP row to the whole row (row_newbcast:k, gfx90a+):
// one v_mov_b64 with a 64-bit DPP source. The DPP control must be an immediate: the
// switch folds away once the callers' fully unrolled loops make k a constant.
// (s_nop 1: a DPP source written by the previous VALU instruction needs two wait
// states, which the compiler does not count for inline assembly.)
template <int K>
__device__ __forceinline__ double bcast16_(double v) {
  double r;
  asm("s_nop 1\n\tv_mov_b64_dpp %0, %1 row_newbcast:%2 row_mask:0xf bank_mask:0xf" : "=v"(r) : "v"(v), "i"(K));
  return r;
}
// acc + (lane k's src) * mul (NEG: - ...), one v_fmac_f64 whose first source is the
// row_newbcast:k DPP operand: a pivot chain's rank-1 update step, or a substitution
// step, without a separate broadcast (fused multiply-add: the same rounding as
// acc - b * mul written out)
template <int K, bool NEG>
__device__ __forceinline__ double fmac_bcast16_(double acc, double src, double mul) {
  if (NEG)
    asm("s_nop 1\n\tv_fmac_f64_dpp %0, %1, -%2 row_newbcast:%3 row_mask:0xf bank_mask:0xf"
                 : "+v"(acc) : "v"(src), "v"(mul), "i"(K));
  else
    asm("s_nop 1\n\tv_fmac_f64_dpp %0, %1, %2 row_newbcast:%3 row_mask:0xf bank_mask:0xf"
                 : "+v"(acc) : "v"(src), "v"(mul), "i"(K));
  return acc;
}
#define MFGP_BCAST16_CASES(F) \
  F(0) F(1) F(2) F(3) F(4) F(5) F(6) F(7) F(8) F(9) F(10) F(11) F(12) F(13) F(14)
__device__ __forceinline__ double bcast16(double v, int k) {
  switch (k) {
#define C_(K) case K: return bcast16_<K>(v);
    MFGP_BCAST16_CASES(C_)
#undef C_
    default: return bcast16_<15>(v);
  }
}
template <bool NEG>
__device__ __forceinline__ double fmac_bcast16(double acc, double src, double mul, int k) {
  switch (k) {
#define C_(K) case K: return fmac_bcast16_<K, NEG>(acc, src, mul);
    MFGP_BCAST16_CASES(C_)
#undef C_
    default: return fmac_bcast16_<15, NEG>(acc, src, mul);
  }
}

// 16x16 f64 MFMA block product on LDS operands: acc (+/-)= A[16xK] * B[Kx16] with
// A[i][k] = A[i*ars + k*acs], B[k][j] = B[k*brs + j*bcs].
template <bool NEG>
__device__ __forceinline__ d4 mfma16(const double* __restrict__ A, int ars, int acs, const double* __restrict__ B,
                                     int brs, int bcs, int K, d4 acc, int lane) {
  const int r = lane & 15, q = lane >> 4;
  for (int k0 = 0; k0 < K; k0 += 4) {
    double a = A[r * ars + (k0 + q) * acs];
    if (NEG) a = -a;
    acc = mfma(a, B[(k0 + q) * brs + r * bcs], acc);
  }
  return acc;
}

// S: 64x64 row-major (stride SP), lower triangle = the matrix. On exit S = L
// (zeros above the diagonal) and R = L^-1 (row-major, zeros above).
#ifndef STAMP   // diagnostic phase stamps: mfgp_kernels.hip defines them for its own build
#define STAMP(id) \
  do {            \
  } while (0)
#endif
__device__ inline void factor_invert_64(double* __restrict__ S, double* __restrict__ R,
                                 double* __restrict__ U, int64_t g0, int64_t N, int* status) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int r16 = lane & 15, q16 = lane >> 4;
  for (int kk = 0; kk < NB / DB; ++kk) {
    const int o = kk * DB;
    if (w == 0) {
      // (a) factor the 16x16 diagonal block in registers: lane r holds row o+(r&15)
      //     (the four 16-lane DPP rows of the wave hold identical copies); column
      //     values are broadcast inside each DPP row with row_newbcast, so no
      //     SGPR/LDS round trip sits on the pivot chain. LAPACK dpotf2 order:
      //     pivot = sqrt(a_jj), column scaled by 1/pivot.
      double d[DB];
#pragma unroll
      for (int c = 0; c < DB; ++c) d[c] = S[(o + r16) * SP + o + c];
      double rdiag = 1.0;
      int fail = INT_MAX;
#pragma unroll
      for (int j = 0; j < DB; ++j) {
        double p = bcast16(d[j], j);
        const int64_t g = g0 + o + j;
        const bool pad = g >= N;
        const bool bad = !pad && !(p > 0.0);
        fail = bad ? min(fail, (int)(g + 1)) : fail;
        p = (pad || bad) ? 1.0 : p;
        const double rs = rsqrt(p);
        const double l = (r16 >= j) ? (r16 == j ? p : d[j]) * rs : 0.0;
        rdiag = (r16 == j) ? rs : rdiag;
        d[j] = l;
        // d[k] -= l_r l_k for every row r: rows r > j are the update; rows r < j have
        // l_r = 0; row j's columns k > j are above the diagonal (never read: the
        // store below and the substitution read columns <= the row)
#pragma unroll
        for (int k = j + 1; k < DB; ++k) d[k] = fmac_bcast16<true>(d[k], l, l, k);
      }
      if (fail != INT_MAX && lane == 0) atomicMin(status, fail);
      if (lane < DB) {
#pragma unroll
        for (int c = 0; c < DB; ++c) S[(o + lane) * SP + o + c] = (c <= lane) ? d[c] : 0.0;
      }
      // inverse of the 16x16 factor: lane c solves column c = r16 by forward
      // substitution; L[i][m] is register m of DPP-row lane i.
      double x[DB];
#pragma unroll
      for (int i = 0; i < DB; ++i) {
        double s0 = (i == r16) ? 1.0 : 0.0, s1 = 0.0;
#pragma unroll
        for (int m = 0; m < i; ++m) {   // s -= L[i][m] x[m]
          if (m & 1) s1 = fmac_bcast16<true>(s1, d[m], x[m], i);
          else s0 = fmac_bcast16<true>(s0, d[m], x[m], i);
        }
        x[i] = (s0 + s1) * bcast16(rdiag, i);
      }
      // column c of Dinv (zero above the diagonal) into R's diagonal block
      if (lane < DB) {
#pragma unroll
        for (int i = 0; i < DB; ++i) R[(o + i) * SP + o + lane] = x[i];
      }
    } else if (kk == 0) {
      // the other waves meanwhile: R's blocks above the diagonal are zero
      for (int e = tid - 64; e < 6 * DB * DB; e += NT - 64) {
        const int b = e >> 8, i = (e >> 4) & 15, j = e & 15;   // blocks (0,1..3), (1,2..3), (2,3)
        const int I = b < 3 ? 0 : (b < 5 ? 1 : 2), J = b < 3 ? b + 1 : (b < 5 ? b - 1 : 3);
        R[(I * DB + i) * SP + J * DB + j] = 0.0;
      }
    }
    __syncthreads();
    STAMP(2 + 3 * kk);
    const int nrest = NB / DB - 1 - kk;   // 16-row blocks below the diagonal block
    // (b) sub-panel P = A_sub * Dinv^T, one 16x16 block per wave (MFMA)
    if (w < nrest) {
      const int R0 = o + DB + DB * w;
      d4 acc = {0.0, 0.0, 0.0, 0.0};
      acc = mfma16<false>(S + R0 * SP + o, SP, 1, R + o * SP + o, 1, SP, DB, acc, lane);   // B[k][j] = Dinv[j][k]
#pragma unroll
      for (int v = 0; v < 4; ++v) S[(R0 + q16 + 4 * v) * SP + o + r16] = acc[v];
    }
    __syncthreads();
    STAMP(3 + 3 * kk);
    // (c) trailing update of the lower 16x16 blocks of rows/cols [o+16, 64) (MFMA)
    for (int t = w; t < nrest * (nrest + 1) / 2; t += NT / 64) {
      int bi = 0;
      while ((bi + 1) * (bi + 2) / 2 <= t) ++bi;
      const int bj = t - bi * (bi + 1) / 2;
      const int R0 = o + DB + DB * bi, C0 = o + DB + DB * bj;
      d4 acc;
#pragma unroll
      for (int v = 0; v < 4; ++v) acc[v] = S[(R0 + q16 + 4 * v) * SP + C0 + r16];
      acc = mfma16<true>(S + R0 * SP + o, SP, 1, S + C0 * SP + o, 1, SP, DB, acc, lane);
#pragma unroll
      for (int v = 0; v < 4; ++v) S[(R0 + q16 + 4 * v) * SP + C0 + r16] = acc[v];
    }
    __syncthreads();
    STAMP(4 + 3 * kk);
  }
  // Linv: the diagonal blocks are in R (and the blocks above them zero); block rows
  // I = 1..3 by substitution:
  //   Linv_IJ = -Dinv_I * sum_{m=J}^{I-1} L_Im Linv_mJ      (MFMA, wave w -> J = w)
  STAMP(14);
  for (int I = 1; I < NB / DB; ++I) {
    if (w < I) {
      const int J = w;
      d4 acc = {0.0, 0.0, 0.0, 0.0};
      acc = mfma16<false>(S + (I * DB) * SP + J * DB, SP, 1, R + (J * DB) * SP + J * DB, SP, 1, (I - J) * DB, acc,
                          lane);
      double* Uj = U + J * DB * DP;
#pragma unroll
      for (int v = 0; v < 4; ++v) Uj[(q16 + 4 * v) * DP + r16] = acc[v];
      __builtin_amdgcn_s_waitcnt(0xc07f);
      __builtin_amdgcn_wave_barrier();
      d4 acc2 = {0.0, 0.0, 0.0, 0.0};
      acc2 = mfma16<true>(R + (I * DB) * SP + I * DB, SP, 1, Uj, DP, 1, DB, acc2, lane);   // Dinv_I
#pragma unroll
      for (int v = 0; v < 4; ++v) R[(I * DB + q16 + 4 * v) * SP + J * DB + r16] = acc2[v];
    }
    __syncthreads();
    STAMP(14 + I);
  }
}

// ---------------------------------------------------------------------------
// The left-looking forward substitution of k_predict (mfgp_kernels.hip) and of the
// look-ahead kernels (mfgp_look.hip): ring constants, LDS-DMA forms, MFMA steps.
// ---------------------------------------------------------------------------
constexpr int KS = 16;                   // K depth of one pipeline step
constexpr int NSTAGE = 3;
constexpr int STAGE = KS * PW + KS * PBM;   // doubles per stage: As [KS][128] + Bs [KS][64]
constexpr int GLDS_PER_STEP = (KS + KS * PBM / 128) / (PNT / 64);   // per wave: 4 (L) + 2 (V)

// Buffer-descriptor LDS-DMA (buffer_load_dwordx4 ... lds): the lane part of the
// source offset is a VGPR fixed for the whole kernel, the row/step part an SGPR,
// so one DMA costs an s_mov to M0 and the load -- no per-row address VALU.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const double* base, int64_t bytes) {
  return __builtin_amdgcn_make_buffer_rsrc((void*)base, 0, (int)(bytes > 0x7fffffff ? 0x7fffffff : bytes), 0x00020000);
}

__device__ __forceinline__ void dma_buf(__amdgpu_buffer_rsrc_t rs, double* dst, unsigned voff, unsigned soff) {
  __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lds_vptr)dst, 16, voff, soff, 0, 0);
}
// the same with the sc1 cache policy (aux 16): served by L2, never by a possibly
// stale line of this CU's L1 -- for bytes another workgroup stored in this launch
__device__ __forceinline__ void dma_buf_sc1(__amdgpu_buffer_rsrc_t rs, double* dst, unsigned voff, unsigned soff) {
  __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lds_vptr)dst, 16, voff, soff, 0, 16);
}


// Main-loop accumulator: wave wm owns rows wm*32.. x all 64 cells.
struct AccP {
  d4 c[2][4];
};
// Diagonal-step accumulator: wave owns 16 rows of a 64-row half x 64 cells.
struct AccH {
  d4 c[4];
};

// acc += A[32 rows of this wave][KS] * B[KS][64]  (acc holds -psi + sum L V)
__device__ __forceinline__ void main_mma(const double* __restrict__ As, const double* __restrict__ Bs, AccP& acc,
                                         int wm, int lane) {
  const int r = lane & 15, q = lane >> 4;
#pragma unroll
  for (int k0 = 0; k0 < KS; k0 += 4) {
    const int k = k0 + q;
    double a[2], b[4];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) a[mt] = As[swzp(k, wm * 32 + mt * 16 + r)];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) b[nt] = Bs[swz(k, nt * 16 + r)];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) acc.c[mt][nt] = mfma(a[mt], b[nt], acc.c[mt][nt]);
  }
}

// A fragments of a column-major 64x64 block (A[i][k] = G[k*lda + i]) for the 16
// rows p16.. of this wave, all 16 K steps: frag[t] = A[p16 + r][4t + q].
__device__ __forceinline__ void load_afrag(double* frag, const double* __restrict__ G, int64_t lda, int p16,
                                           int lane) {
  const int r = lane & 15, q = lane >> 4;
#pragma unroll
  for (int t = 0; t < 16; ++t) frag[t] = gp(G)[(int64_t)(4 * t + q) * lda + p16 + r];
}

// acc (+/-)= A[16 x 4*nt4] (fragments) * img[rows rb..][64 cells]; nt4 K steps
template <bool NEG>
__device__ __forceinline__ void half_mma(const double* frag, const double* __restrict__ img, int rb, AccH& acc,
                                         int nt4, int lane) {
  const int r = lane & 15, q = lane >> 4;
#pragma unroll
  for (int t = 0; t < 16; ++t) {
    if (t < nt4) {
      const double a = NEG ? -frag[t] : frag[t];
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) acc.c[nt] = mfma(a, img[swz(rb + 4 * t + q, nt * 16 + r)], acc.c[nt]);
    }
  }
}

}  // namespace mfgp
