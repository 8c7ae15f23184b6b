// Look-ahead variance and off-grid queries for gfx950 (MI355X), fp64.
//
// Reference: MFGP.pred_var (gaussian_process.py:440-481) stacks prospective rows
// X_L_new / X_H_new under the training set, refactors all N + P rows and returns the
// dense covariance at x; get_neg_var / get_max_var (gp:544-578) call it per point.
// The factor L of the N current rows, the inverses of its diagonal blocks and
// z = L^-1 (y - m) are resident, the posterior does not depend on row order, and
// prospective rows carry no values, so with the P <= 64 prospective rows behind
// the N current ones:
//   k_look_border  (one workgroup, once per prospective set)
//       W = L^-1 K(X, X_P)                      [N x P], the L21^T block of the border
//       S = K(X_P, X_P) + noise + jitter - W^T W,   L22 = chol(S),   L22^-1
//   k_look_query   (one workgroup per 64 query points q)
//       v = L^-1 psi_q,   mu = m_H + v^T z,   var0 = k** - |v|^2      (the current model)
//       t = L22^-1 (K(X_P, q) - W^T v),       var = var0 - |t|^2      (with the border)
//     and, for the dense covariance, the rows of t behind the rows of v in the
//     scratch tile, which k_cov_block (mfgp_cov.hip) then reads as a V of N + P rows.
// Both kernels run look_subst: k_predict's left-looking blocked forward substitution
// (mfgp_kernels.hip; the shared steps live in mfgp_device.h) over a list of points
// with a fidelity per column instead of grid cells. A tile's rows are stored to and
// re-read from a tile [vld][64] that the caller provides (the record's W, or context
// workspace): the model's resident V is never touched. No flags, atomics across
// workgroups or hand-offs: border, query and covariance are consecutive launches.
// A column's results depend on its own point only (fixed reduction order, padding
// columns are clamped copies), so a query's bits do not depend on its batch.
#include <climits>
#include <hip/hip_runtime.h>

#include "mfgp_device.h"
#include "mfgp_internal.h"

namespace mfgp {

// A point's coordinates over both length scales (x / l before the subtraction, gp:77-78).
struct LookPt {
  double xL, yL, xH, yH;
};
__device__ __forceinline__ LookPt look_pt(const Hyp& h, const double* __restrict__ pts, int64_t i) {
  const double x = gp(pts)[2 * i], y = gp(pts)[2 * i + 1];
  LookPt p;
  p.xL = div_(x, h.lL);
  p.yL = div_(y, h.lL);
  p.xH = div_(x, h.lH);
  p.yH = div_(y, h.lH);
  return p;
}

// Covariance of two rows by their fidelities (gp:465-468 / 473-475; SF: the one
// kernel): lofi-lofi k_L, lofi-hifi rho k_L, hifi-hifi rho^2 k_L + k_H -- the
// operation order of k_entry_pts and of k_predict's psi, no FMA contraction.
__device__ __forceinline__ double look_k(const Hyp& h, bool lo_a, const LookPt& a, bool lo_b, const LookPt& b) {
#pragma clang fp contract(off)
  const double kl = se_scaled(a.xL, a.yL, b.xL, b.yL, h.sL);
  if (h.kind == 0 || (lo_a && lo_b)) return kl;
  if (lo_a != lo_b) return h.rho * kl;
  const double kh = se_scaled(a.xH, a.yH, b.xH, b.yH, h.sH);
  return h.rho2 * kl + kh;
}
// The same for the four columns of a lane against one training row, branching on
// the row alone (k_predict's psi); FID: the columns have fidelities (else all hifi).
template <bool FID>
__device__ __forceinline__ void look_psi4(const Hyp& h, const bool* clo, const LookPt* cp, bool tlo, const LookPt& tp,
                                          double* pv) {
#pragma clang fp contract(off)
  if (h.kind == 0) {
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) pv[nt] = se_scaled(cp[nt].xL, cp[nt].yL, tp.xL, tp.yL, h.sL);
  } else if (tlo) {
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
      const double kl = se_scaled(cp[nt].xL, cp[nt].yL, tp.xL, tp.yL, h.sL);
      const double rk = h.rho * kl;
      pv[nt] = (FID && clo[nt]) ? kl : rk;
    }
  } else {
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
      const double kl = se_scaled(cp[nt].xL, cp[nt].yL, tp.xL, tp.yL, h.sL);
      const double kh = se_scaled(cp[nt].xH, cp[nt].yH, tp.xH, tp.yH, h.sH);
      const double hh = h.rho2 * kl + kh;
      const double rk = h.rho * kl;
      pv[nt] = (FID && clo[nt]) ? rk : hh;
    }
  }
}

// Per lane: the partial sums of |v|^2 and v^T z of its four columns nt * 16 + r over
// the rows of its class (wave w, row group q) -- the rows k_predict's lane sums, in
// its order (blocks ascending, the top half's four rows, then the bottom half's; its
// a += x * y are fused multiply-adds).
struct LookSums {
  double vsum[4], msum[4];
};
__device__ __forceinline__ void look_sums(const double* __restrict__ Vt, const double* __restrict__ zv, int64_t N,
                                          int w, int q, int r, LookSums& s) {
#pragma unroll
  for (int nt = 0; nt < 4; ++nt) s.vsum[nt] = s.msum[nt] = 0.0;
  for (int64_t base = 0; base < N; base += PRB) {
#pragma unroll
    for (int hv = 0; hv < 8; ++hv) {
      const int64_t row = base + (hv >> 2) * NB + w * 16 + q + 4 * (hv & 3);
      if (row < N) {
        const double z = gp(zv)[row];
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
          const double val = gp(Vt)[row * PBM + nt * 16 + r];
          s.vsum[nt] = fma(val, val, s.vsum[nt]);
          s.msum[nt] = fma(val, z, s.msum[nt]);
        }
      }
    }
  }
}

// V = L^-1 psi^T for the 64 columns c0 .. c0 + 63 of the point list `pts` (FID: fid[c] = 0
// for a lofi row, 1 for hifi; else all hifi), rows [0, N) stored to Vt[row * 64 + column].
// lds: NSTAGE * STAGE doubles. Ends behind a barrier with all stores complete. The
// sums over the rows are taken afterwards from the stored tile (look_sums): carried
// through this loop they would not fit the 256 registers of two workgroups per CU.
template <bool FID>
__device__ __forceinline__ void look_subst(const LookArgs& a, const double* __restrict__ pts,
                                           const int* __restrict__ fid, int64_t M, int64_t c0,
                                           double* __restrict__ Vt, double* lds) {
  double* const img = lds;
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave id (uniform)
  const int r = lane & 15, q = lane >> 4;
  const int p16 = w * 16;   // diagonal-step rows of this wave inside a 64-row half
  const Hyp& h = a.h;
  const int64_t N = a.N, NL = a.NL, ld = a.ld;
  const int64_t nrb = prow_blocks(N);
  const int64_t nbf = nblocks_factor(N);
  const double* __restrict__ X = a.X;
  const double* __restrict__ Amat = a.A;
  // the DMA plan of one K step: k_predict's
  const __amdgpu_buffer_rsrc_t rsA = make_rsrc(Amat, (int64_t)8 * ld * ld);
  const __amdgpu_buffer_rsrc_t rsV = make_rsrc(Vt, (int64_t)8 * a.vld * PBM);
  const unsigned voffA = (unsigned)(8 * ((2 * lane) ^ ((w & 1) << 4)));
  const unsigned voffV = (unsigned)(8 * ((lane >> 5) * PBM + (((lane & 31) * 2) ^ ((lane >> 5) << 4))));
  auto dma_step = [&](double* st, int64_t base_, int64_t kc) {
#pragma unroll
    for (int j = 0; j < KS / 4; ++j) {
      const int k = w + 4 * j;
      dma_buf(rsA, st + k * PW, voffA, (unsigned)(8 * ((kc + k) * ld + base_)));
    }
#pragma unroll
    for (int j = 0; j < KS / 8; ++j) {
      const int pp = w + 4 * j;
      dma_buf(rsV, st + KS * PW + 2 * pp * PBM, voffV, (unsigned)(8 * (kc + 2 * pp) * PBM));
    }
  };

  for (int64_t I = 0; I < nrb; ++I) {
    const int64_t base = I * PRB;
    const int nk = (int)(base / KS);   // K steps: all columns left of the block (rows < base <= N)
    const int nin = (int)(N - base < PRB ? N - base : PRB);   // the block's rows below N
    double* const Vb = Vt + base * PBM;
#pragma unroll
    for (int s0 = 0; s0 < 2; ++s0) {
      if (s0 < nk) dma_step(lds + s0 * STAGE, base, (int64_t)s0 * KS);
    }
    AccP acc;
    {
      // this lane's four columns nt * 16 + r (past the list: clamped copies of its last
      // point), loaded and scaled per block as k_predict does so that they are not live
      // across the K loop (the opaque lane offset keeps the loads inside the block loop)
      LookPt cp[4];
      bool clo[4];
      int rr = r;
      asm volatile("" : "+v"(rr));
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) {
        int64_t c = c0 + nt * 16 + rr;
        if (c >= M) c = M - 1;
        cp[nt] = look_pt(h, pts, c);
        clo[nt] = FID ? (gp(fid)[c] == 0) : false;
      }
#pragma unroll
      for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          const int64_t g = base + w * 32 + mt * 16 + q + 4 * v;
          double pv[4] = {0.0, 0.0, 0.0, 0.0};
          if (g < N) {   // rows >= N of A (the residual row, the padding) are no training rows
            const LookPt tp = look_pt(h, X, g);
            const bool tlo = g < NL;
            look_psi4<FID>(h, clo, cp, tlo, tp, pv);
          }
#pragma unroll
          for (int nt = 0; nt < 4; ++nt) acc.c[mt][nt][v] = -pv[nt];   // acc = -psi + sum L V
        }
    }
    double frag[16];
    if (nk > 0) {
      if (nk > 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(GLDS_PER_STEP) : "memory");
      else vm_wait_all();
      __builtin_amdgcn_s_barrier();
    }
    for (int s = 0; s < nk; ++s) {
      const double* cur = lds + (s % NSTAGE) * STAGE;
      if (s + 2 < nk) dma_step(lds + ((s + 2) % NSTAGE) * STAGE, base, (int64_t)(s + 2) * KS);
      main_mma(cur, cur + KS * PW, acc, w, lane);
      if (s + 2 < nk) asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"(GLDS_PER_STEP) : "memory");
      else asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");
    }
    // ---- diagonal block: V_I = L_II^-1 (psi - L V), two 64-row halves ----
    const int64_t fa = 2 * I, fb = 2 * I + 1;
    const bool has_b = fb < nbf;
    load_afrag(frag, a.Linv + fa * TILE, NB, p16, lane);   // Linv_a
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int nt = 0; nt < 4; ++nt)
#pragma unroll
        for (int v = 0; v < 4; ++v) img[swz(w * 32 + mt * 16 + q + 4 * v, nt * 16 + r)] = -acc.c[mt][nt][v];
    __syncthreads();
    AccH vh;
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) vh.c[nt] = d4{0.0, 0.0, 0.0, 0.0};
    half_mma<false>(frag, img, 0, vh, (p16 + 16) / 4, lane);
    if (has_b) {
      // (an opaque copy of ld: the 16 row offsets (4t + q) * ld are recomputed here
      // instead of living in registers across the block loop)
      int64_t ldo = ld;
      asm volatile("" : "+s"(ldo));
      load_afrag(frag, Amat + fa * NB * ld + fb * NB, ldo, p16, lane);   // L_ba
    }
#pragma unroll
    for (int nt = 0; nt < 4; ++nt)
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int row = p16 + q + 4 * v, col = nt * 16 + r;
        const double val = vh.c[nt][v];
        if (row < nin) gp(Vb)[row * PBM + col] = val;
      }
    __syncthreads();   // every wave is done reading T_top
    if (has_b) {
#pragma unroll
      for (int nt = 0; nt < 4; ++nt)
#pragma unroll
        for (int v = 0; v < 4; ++v) img[swz(p16 + q + 4 * v, nt * 16 + r)] = vh.c[nt][v];
      __syncthreads();
      AccH th;
#pragma unroll
      for (int nt = 0; nt < 4; ++nt)
#pragma unroll
        for (int v = 0; v < 4; ++v) th.c[nt][v] = img[swz(64 + p16 + q + 4 * v, nt * 16 + r)];
      half_mma<true>(frag, img, 0, th, 16, lane);
      load_afrag(frag, a.Linv + fb * TILE, NB, p16, lane);   // Linv_b
#pragma unroll
      for (int nt = 0; nt < 4; ++nt)
#pragma unroll
        for (int v = 0; v < 4; ++v) img[swz(64 + p16 + q + 4 * v, nt * 16 + r)] = th.c[nt][v];
      __syncthreads();
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) vh.c[nt] = d4{0.0, 0.0, 0.0, 0.0};
      half_mma<false>(frag, img, 64, vh, (p16 + 16) / 4, lane);
#pragma unroll
      for (int nt = 0; nt < 4; ++nt)
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          const int row = 64 + p16 + q + 4 * v, col = nt * 16 + r;
          const double val = vh.c[nt][v];
          if (row < nin) gp(Vb)[row * PBM + col] = val;
        }
    }
    vm_wait_all();      // V_I stores complete before any later DMA (or load) reads them
    __syncthreads();    // and before the next prologue overwrites the LDS images
  }
}

// Ts[swz(k, i)] = G[(n0 + k) * 64 + i] for rows n0 + k < N, zeros below: 64 rows of a
// [rows][64] tile as a k-major MFMA operand (rows >= N may hold an older call's values).
__device__ __forceinline__ void look_put_rows(double* __restrict__ Ts, const double* __restrict__ G, int64_t n0,
                                              int64_t N, int tid) {
#pragma unroll
  for (int p = 0; p < 8; ++p) {
    const int k = p * 8 + (tid >> 5), i = (tid & 31) * 2;
    dv2 v = {0.0, 0.0};
    if (n0 + k < N) v = *reinterpret_cast<const GLOBAL dv2*>(gp(G) + (n0 + k) * PBM + i);
    *reinterpret_cast<dv2*>(Ts + swz(k, i)) = v;
  }
}

// The border of the P = a.P prospective points a.ppts / a.pfid (1 <= P <= 64, padded to
// 64 columns by copies of the last): W into a.W, L22 and L22^-1 (column-major, identity
// on rows and columns >= P) into the record, *a.status = INT_MAX or 1 + the first
// non-positive pivot's row. One workgroup.
__global__ __launch_bounds__(PNT, 2) void k_look_border(const LookArgs a) {
  __shared__ double lds[NSTAGE * STAGE];
  static_assert(2 * NB * SP + (NB / DB - 1) * DB * DP <= NSTAGE * STAGE, "the factor's tiles fit the ring");
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int wm = w >> 1, wn = w & 1;
  const int r = lane & 15, q = lane >> 4;
  const int P = a.P;
  if (tid == 0) *a.status = INT_MAX;   // (this thread also issues the factor's atomicMin on it)
  look_subst<true>(a, a.ppts, a.pfid, P, 0, a.W, lds);
  // S = W^T W over the N rows: both operands the same image
  Acc acc;
  acc_zero(acc);
  for (int64_t n0 = 0; n0 < a.N; n0 += NB) {
    look_put_rows(lds, a.W, n0, a.N, tid);
    __syncthreads();
    tile_mma<false>(lds, lds, acc, wm, wn, lane);
    __syncthreads();
  }
  double* const S = lds;
  double* const R = lds + NB * SP;
  double* const U = R + NB * SP;
  const Hyp& h = a.h;
#pragma unroll
  for (int mt = 0; mt < 2; ++mt)
#pragma unroll
    for (int v = 0; v < 4; ++v)
#pragma unroll
      for (int nt = 0; nt < 2; ++nt) S[acc_row(wm, mt, q, v) * SP + acc_col(wn, nt, r)] = acc.c[mt][nt][v];
  __syncthreads();
  {
    // K_PP + noise + jitter - W^T W on the P x P corner, identity beyond; thread: column
    // j, rows i = w + 4 it (one K entry at a time: few registers)
    const int j = lane, jc = j < P ? j : P - 1;
    const double pj[2] = {gp(a.ppts)[2 * jc], gp(a.ppts)[2 * jc + 1]};
    const int64_t gj = gp(a.pfid)[jc] ? NB + j : j;   // k_entry_pts: rows below "NL" = NB are lofi
#pragma unroll 1
    for (int i = w; i < NB; i += PNT / 64) {
      const int ic = i < P ? i : P - 1;
      const double pi[2] = {gp(a.ppts)[2 * ic], gp(a.ppts)[2 * ic + 1]};
      const int64_t gi = gp(a.pfid)[ic] ? NB + i : i;
      double s = (i == j) ? 1.0 : 0.0;
      if (i < P && j < P) s = k_entry_pts(h, NB, gi, pi, gj, pj) - S[i * SP + j];
      S[i * SP + j] = (j <= i) ? s : 0.0;
    }
  }
  __syncthreads();
  factor_invert_64(S, R, U, 0, P, a.status);
#pragma unroll 4
  for (int e = tid; e < NB * NB; e += PNT) {
    const int i = e & 63, j = e >> 6;   // column-major, as Linv's blocks
    gp(a.L22)[j * NB + i] = S[i * SP + j];
    gp(a.L22inv)[j * NB + i] = R[i * SP + j];
  }
}

// mu / var0 / var (each or null) of the query points a.pts[0 .. a.M): one workgroup
// per 64. a.P = 0: no border (var = var0). a.store_t: the P rows of t go behind the N
// rows of v in the scratch tile (rows N .. N + P - 1), for k_cov_block.
__global__ __launch_bounds__(PNT, 2) void k_look_query(const LookArgs a) {
  __shared__ double lds[NSTAGE * STAGE];
  const int64_t c0 = (int64_t)blockIdx.x * PBM;
  if (c0 >= a.M) return;
  const int P = a.P;
  const int64_t N = a.N;
  const Hyp& h = a.h;
  double* __restrict__ Vt = a.scr + (int64_t)blockIdx.x * a.vld * PBM;
  look_subst<false>(a, a.pts, nullptr, a.M, c0, Vt, lds);
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int wm = w >> 1, wn = w & 1;
  const int r = lane & 15, q = lane >> 4;
  const int p16 = w * 16;
  LookSums sums;
  look_sums(Vt, a.zv, N, w, q, r, sums);
  double tsum[4] = {0.0, 0.0, 0.0, 0.0};
  if (P > 0) {
    // T = K(X_P, q) - W^T v: K loop over the N rows, A operand the record's W
    double* const As = lds;
    double* const Bs = lds + TILE;
    Acc acc;
    acc_zero(acc);
    for (int64_t n0 = 0; n0 < N; n0 += NB) {
      look_put_rows(As, a.W, n0, N, tid);
      look_put_rows(Bs, Vt, n0, N, tid);
      __syncthreads();
      tile_mma<true>(As, Bs, acc, wm, wn, lane);
      __syncthreads();
    }
    double* const img = lds;
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int v = 0; v < 4; ++v)
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) img[swz(acc_row(wm, mt, q, v), acc_col(wn, nt, r))] = acc.c[mt][nt][v];
    __syncthreads();
    {
      // T = K(X_P, q) - W^T v; thread: column lane, rows p = w + 4 it (one K entry at a
      // time: few registers); rows >= P contribute nothing
      const int64_t c = c0 + lane < a.M ? c0 + lane : a.M - 1;
      const LookPt qp = look_pt(h, a.pts, c);
#pragma unroll 1
      for (int p = w; p < NB; p += PNT / 64) {
        double t = 0.0;
        if (p < P) {
          const LookPt pp = look_pt(h, a.ppts, p);
          t = look_k(h, false, qp, gp(a.pfid)[p] == 0, pp) + img[swz(p, lane)];
        }
        img[swz(p, lane)] = t;
      }
    }
    double frag[16];
    load_afrag(frag, a.L22inv, NB, p16, lane);
    __syncthreads();
    // t = L22^-1 T (lower triangular: rows p16.. need K < p16 + 16)
    AccH th;
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) th.c[nt] = d4{0.0, 0.0, 0.0, 0.0};
    half_mma<false>(frag, img, 0, th, (p16 + 16) / 4, lane);
#pragma unroll
    for (int nt = 0; nt < 4; ++nt)
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int row = p16 + q + 4 * v, col = nt * 16 + r;
        const double val = th.c[nt][v];
        if (row < P) {
          tsum[nt] += val * val;
          if (a.store_t) gp(Vt)[(N + row) * PBM + col] = val;
        }
      }
    __syncthreads();   // every wave is done reading T
  }
  // the four row classes of a wave, then the four waves: ((0 + 1) + (2 + 3)), k_predict's order
#pragma unroll
  for (int nt = 0; nt < 4; ++nt) {
    sums.vsum[nt] += __shfl_xor(sums.vsum[nt], 16);
    sums.vsum[nt] += __shfl_xor(sums.vsum[nt], 32);
    sums.msum[nt] += __shfl_xor(sums.msum[nt], 16);
    sums.msum[nt] += __shfl_xor(sums.msum[nt], 32);
    tsum[nt] += __shfl_xor(tsum[nt], 16);
    tsum[nt] += __shfl_xor(tsum[nt], 32);
  }
  double* red = lds;   // [3][4][PBM]
  if (q == 0) {
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
      red[(0 * 4 + w) * PBM + nt * 16 + r] = sums.vsum[nt];
      red[(1 * 4 + w) * PBM + nt * 16 + r] = sums.msum[nt];
      red[(2 * 4 + w) * PBM + nt * 16 + r] = tsum[nt];
    }
  }
  __syncthreads();
  if (tid < PBM) {
    const int64_t c = c0 + tid;
    const double vs = (red[0 * PBM + tid] + red[1 * PBM + tid]) + (red[2 * PBM + tid] + red[3 * PBM + tid]);
    const double ms = (red[4 * PBM + tid] + red[5 * PBM + tid]) + (red[6 * PBM + tid] + red[7 * PBM + tid]);
    const double ts = (red[8 * PBM + tid] + red[9 * PBM + tid]) + (red[10 * PBM + tid] + red[11 * PBM + tid]);
    const double v0 = h.kss - vs;
    if (c < a.M) {
      if (a.mu) gp(a.mu)[c] = ms + h.meanH;
      if (a.var0) gp(a.var0)[c] = v0;
      if (a.var) gp(a.var)[c] = v0 - ts;
    }
  }
}

hipError_t launch_look_border(const LookArgs& a, hipStream_t s) {
  if (a.P <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_look_border, dim3(1), dim3(PNT), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_look_query(const LookArgs& a, hipStream_t s) {
  if (a.M <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_look_query, dim3((unsigned)ntiles_grid(a.M)), dim3(PNT), 0, s, a);
  return hipGetLastError();
}

}  // namespace mfgp
