// Blocks of the dense posterior covariance for gfx950 (MI355X), fp64.
//
// Reference: SFGP.predict / MFGP.predict return the dense [M,M] covariance
// (gaussian_process.py:146, 435-436):
//   cov = k**(X*, X*) - psi K^-1 psi^T = k**(X*, X*) - V^T V,   V = L^-1 psi^T
// V is resident per model after every predict path ([tile][vld][64 cells], rows
// [0, N) valid), so a block cov[rows, cols] is one GEMM over V's rows plus the
// prior term:
//   k_cov_block   one workgroup per 64x64 output tile, four waves of 32x32 on
//                 v_mfma_f64_16x16x4; K loop over the training rows in chunks of
//                 64, both operand panels gathered through LDS (lane -> cell, so
//                 a contiguous index list reads V's 512-byte rows whole)
// Every output entry accumulates the products V[n,i] V[n,j] in the same order
// (n ascending, no split-K, no atomics) whatever its place in a tile, so an
// entry's bits depend only on its pair of cells: block(a, b) == block(b, a)^T
// and any sub-block equals the same entries of the full matrix, bit for bit.
#include <hip/hip_runtime.h>

#include "mfgp_cov.h"

namespace mfgp {

// out[i * ldo + j] = cov(rows[i], cols[j]), i < na, j < nb; rows / cols null = the
// identity list. Grid: (ceil(nb / 64), ceil(na / 64)). prior_only: k** alone.
__global__ __launch_bounds__(NT) void k_cov_block(const GPDesc d, const int64_t* __restrict__ rows, int64_t na,
                                                  const int64_t* __restrict__ cols, int64_t nb,
                                                  double* __restrict__ out, int64_t ldo, int prior_only) {
  __shared__ double As[TILE];
  __shared__ double Bs[TILE];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int wm = w >> 1, wn = w & 1;
  const int64_t i0 = (int64_t)blockIdx.y * 64, j0 = (int64_t)blockIdx.x * 64;
  const int64_t N = prior_only ? 0 : d.N;
  Acc acc;
  acc_zero(acc);
  if (N > 0) {
    const bool oka = i0 + lane < na, okb = j0 + lane < nb;
    const int64_t ca = oka ? (rows ? gp(rows)[i0 + lane] : i0 + lane) : 0;
    const int64_t cb = okb ? (cols ? gp(cols)[j0 + lane] : j0 + lane) : 0;
    const GLOBAL double* pa = gp(d.V) + (ca / PBM) * d.vld * PBM + ca % PBM;
    const GLOBAL double* pb = gp(d.V) + (cb / PBM) * d.vld * PBM + cb % PBM;
    CovStage st;
    cov_fetch(st, pa, pb, oka, okb, 0, N, w);
    for (int64_t n0 = 0; n0 < N; n0 += CKC) {
      cov_put(As, Bs, st, w, lane);
      __syncthreads();
      if (n0 + CKC < N) cov_fetch(st, pa, pb, oka, okb, n0 + CKC, N, w);
      tile_mma<false>(As, Bs, acc, wm, wn, lane);
      __syncthreads();
    }
  }
  const Hyp& h = d.hp;
  const int r = lane & 15, q = lane >> 4;
  CovPt pc[2];
  int64_t jc[2];
#pragma unroll
  for (int nt = 0; nt < 2; ++nt) {
    jc[nt] = j0 + acc_col(wn, nt, r);
    const int64_t cell = jc[nt] < nb ? (cols ? gp(cols)[jc[nt]] : jc[nt]) : 0;
    pc[nt] = cov_pt(h, d.grid, cell);
  }
#pragma unroll
  for (int mt = 0; mt < 2; ++mt)
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int64_t i = i0 + acc_row(wm, mt, q, v);
      if (i >= na) continue;
      const CovPt pr = cov_pt(h, d.grid, rows ? gp(rows)[i] : i);
#pragma unroll
      for (int nt = 0; nt < 2; ++nt)
        if (jc[nt] < nb) gp(out)[i * ldo + jc[nt]] = cov_entry(h, pr, pc[nt], acc.c[mt][nt][v]);
    }
}

hipError_t launch_cov_block(const GPDesc& d, const int64_t* rows, int64_t na, const int64_t* cols, int64_t nb,
                            double* out, int64_t ldo, int prior_only, hipStream_t s) {
  if (na <= 0 || nb <= 0) return hipSuccess;
  const dim3 grid((unsigned)((nb + 63) / 64), (unsigned)((na + 63) / 64));
  hipLaunchKernelGGL(k_cov_block, grid, dim3(NT), 0, s, d, rows, na, cols, nb, out, ldo, prior_only);
  return hipGetLastError();
}

}  // namespace mfgp
