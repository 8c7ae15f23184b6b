// Integrated variance reduction per candidate cell for gfx950 (MI355X), fp64.
//
// Measuring the hifi field at grid cell c lowers the posterior variance of cell i by
// cov(i, c)^2 / (cov(c, c) + sigma_H + jitter) (a rank-one update of the posterior; the
// denominator's noise and jitter are the diagonal term a hifi append adds to K, an SF
// model's single noise). The score of a candidate under a weight vector w over the
// grid's M cells is the A-optimal / integrated-variance criterion
//   IVR_w(c) = sum_i w_i cov(i, c)^2 / d_c,   d_c = cov(c, c) + sigma_H + jitter,
// and cov(i, c) = k**(i, c) - sum_n V[n,i] V[n,c] is k_cov_block's GEMM over the resident
// V = L^-1 psi^T (mfgp_cov.h). The numerator is colsum(w o cov^2), so the kernels below
// reduce the M x C block in registers and it never exists in memory.
//
//   k_ivr_partial  one workgroup per (tile of 64 candidates, row segment). A segment is
//                  IVR_SEG consecutive 64-cell row tiles, so the partition of the rows
//                  depends on M alone. Per row tile, ascending: k_cov_block's K loop
//                  (chunks of 64 training rows, n ascending, no split-K, zeros for rows
//                  >= N and for cells past M or past the candidate list, never loaded),
//                  then e = cov_entry(...) per entry of the tile and
//                  s[k] += w_k[i] * (e * e) into the thread's column sums, k < nw. A row
//                  tile whose weights are zero in all nw vectors is skipped: its terms
//                  are zeros, which change no bits of a sum, so a region mask costs its
//                  region. After the segment the threads' sums meet through LDS and the
//                  workgroup stores partial[segment][k][candidate].
//   k_ivr_finish   one thread per candidate: the denominator, the segments' partials
//                  added in segment order, the division, the store; then the workgroup's
//                  (max, first position in the candidate list) per weight vector.
//   k_ivr_best     one workgroup per weight vector reduces those pairs (argmax_pair's
//                  rule: the larger value, the lower position on ties).
// No atomics, no flags, no calls; three launches on one stream.
//
// Order of sums. After a tile's K loop the accumulators go to LDS, and thread (wave wv,
// lane) owns column `lane` and the rows 16 wv .. 16 wv + 15: it adds its terms row tile after
// row tile of the segment, within a tile rows ascending; a column's four quarter sums are
// then added as wv = 0, 1, 2, 3, starting from the first; the segments' partials are added
// in segment order starting from 0.0. The denominator is
//   vv = 0; for n = 0 .. N-1: vv = fma(V[n,c], V[n,c], vv);
//   d_c = (cov_entry(c, c, vv) + sigma_H) + jitter
// by one thread, n ascending. None of this depends on the candidate's place in the list,
// on the list's length, on the other candidates, on nw or on the other weight vectors,
// so out[k][j] depends bit for bit only on the model, the cell cand[j] and w_k.
#include <hip/hip_runtime.h>

#include "mfgp_cov.h"

namespace mfgp {

// LDS after a tile's K loop. Bs: the tile's V_i . V_j sums, C[row][column]. As: the tile's
// weights Ws[k][row] (8 x 64), then its rows' scaled coordinates (64 x 4, CovPt's order);
// after the segment: the four quarter sums of every column, red[k][quarter][column].
constexpr int IVR_PTS = IVR_MAXW * 64;
__device__ __forceinline__ int ivr_red(int k, int g, int col) { return (k * 4 + g) * 64 + col; }

__global__ __launch_bounds__(NT, 2) void k_ivr_partial(const GPDesc d, const int64_t* __restrict__ cand,
                                                       int64_t nc, const double* __restrict__ w, int nw,
                                                       int64_t ldw, double* __restrict__ partial) {
  __shared__ double As[TILE];
  __shared__ double Bs[TILE];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int wm = wv >> 1, wn = wv & 1;
  const int64_t j0 = (int64_t)blockIdx.x * 64;
  const int64_t M = d.M, N = d.N;
  const Hyp& h = d.hp;
  const int r = lane & 15, q = lane >> 4;
  // candidate j0 + lane: this lane's panel column in the K loop and its column in the epilogue
  const bool okb = j0 + lane < nc;
  const int64_t cb = okb ? (cand ? gp(cand)[j0 + lane] : j0 + lane) : 0;
  const CovPt pc = cov_pt(h, d.grid, cb);
  double s[IVR_MAXW];
#pragma unroll
  for (int k = 0; k < IVR_MAXW; ++k) s[k] = 0.0;

  const int64_t t0 = (int64_t)blockIdx.y * IVR_SEG;
  const int64_t tiles = ntiles_grid(M);
  const int64_t t1 = t0 + IVR_SEG < tiles ? t0 + IVR_SEG : tiles;
  for (int64_t t = t0; t < t1; ++t) {
    const int64_t i0 = t * 64;
    // the tile's weights: thread (wave wv, lane) holds vectors wv and wv + 4 of row i0 + lane;
    // rows past M and vectors past nw weigh nothing
    const bool oka = i0 + lane < M;
    double w0 = 0.0, w1 = 0.0;
    if (oka) {
      if (!w) {
        w0 = wv == 0 ? 1.0 : 0.0;
      } else {
        if (wv < nw) w0 = gp(w)[wv * ldw + i0 + lane];
        if (wv + 4 < nw) w1 = gp(w)[(wv + 4) * ldw + i0 + lane];
      }
    }
    if (!__syncthreads_or(w0 != 0.0 || w1 != 0.0)) continue;
    Acc acc;
    acc_zero(acc);
    if (N > 0) {
      // (the candidate's column of V from an opaque copy of its cell: the 16 row addresses of
      // a chunk are then no invariants of the tile loop, which would hold 32 registers)
      int64_t cbt = cb;
      asm volatile("" : "+v"(cbt));
      const GLOBAL double* pb = gp(d.V) + (cbt / PBM) * d.vld * PBM + cbt % PBM;
      const GLOBAL double* pa = gp(d.V) + t * d.vld * PBM + lane;
      CovStage st;
      cov_fetch(st, pa, pb, oka, okb, 0, N, wv);
      for (int64_t n0 = 0; n0 < N; n0 += CKC) {
        cov_put(As, Bs, st, wv, lane);
        __syncthreads();
        if (n0 + CKC < N) cov_fetch(st, pa, pb, oka, okb, n0 + CKC, N, wv);
        tile_mma<false>(As, Bs, acc, wm, wn, lane);
        __syncthreads();
      }
    }
    // the K loop is done with As and Bs: the sums, the weights and the rows' points go there
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int nt = 0; nt < 2; ++nt)
#pragma unroll
        for (int v = 0; v < 4; ++v) Bs[acc_row(wm, mt, q, v) * 64 + acc_col(wn, nt, r)] = acc.c[mt][nt][v];
    As[wv * 64 + lane] = w0;
    As[(wv + 4) * 64 + lane] = w1;
    {
      // thread tid: coordinate tid & 1 of row tid >> 2 over length scale (tid >> 1) & 1 (cov_pt's
      // four quotients, one per thread)
      const int64_t i = i0 + (tid >> 2);
      const double xy = gp(d.grid)[2 * (i < M ? i : 0) + (tid & 1)];
      As[IVR_PTS + tid] = div_(xy, (tid & 2) ? h.lH : h.lL);
    }
    __syncthreads();
    // thread (wv, lane): rows 16 wv .. 16 wv + 15 of column `lane`, ascending
#pragma unroll 2
    for (int rr = 0; rr < 16; ++rr) {
#pragma clang fp contract(off)
      const int row = wv * 16 + rr;
      CovPt pr;
      pr.xL = As[IVR_PTS + 4 * row];
      pr.yL = As[IVR_PTS + 4 * row + 1];
      pr.xH = As[IVR_PTS + 4 * row + 2];
      pr.yH = As[IVR_PTS + 4 * row + 3];
      const double e = cov_entry(h, pr, pc, Bs[row * 64 + lane]);
      const double e2 = e * e;
#pragma unroll
      for (int k = 0; k < IVR_MAXW; ++k)
        if (k < nw) s[k] = s[k] + As[k * 64 + row] * e2;
    }
    __syncthreads();
  }

  // the four quarter sums of every column, in the order of the rows
#pragma unroll
  for (int k = 0; k < IVR_MAXW; ++k)
    if (k < nw) As[ivr_red(k, wv, lane)] = s[k];
  __syncthreads();
  if (okb) {
    for (int k = wv; k < nw; k += 4) {
      double sum = As[ivr_red(k, 0, lane)];
#pragma unroll
      for (int g = 1; g < 4; ++g) sum = sum + As[ivr_red(k, g, lane)];
      gp(partial)[((int64_t)blockIdx.y * nw + k) * nc + j0 + lane] = sum;
    }
  }
}

// bval / bpos [nw][gridDim.x]: the workgroups' (max, first position)
__global__ __launch_bounds__(NT) void k_ivr_finish(const GPDesc d, const int64_t* __restrict__ cand, int64_t nc,
                                                   const double* __restrict__ partial, int nseg, int nw,
                                                   double* __restrict__ out, int64_t ldo,
                                                   double* __restrict__ bval, int64_t* __restrict__ bpos) {
  __shared__ double rv[4];
  __shared__ int64_t ri[4];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int64_t j = (int64_t)blockIdx.x * NT + tid;
  const bool ok = j < nc;
  const Hyp& h = d.hp;
  double dc = 1.0;
  if (ok) {
#pragma clang fp contract(off)
    const int64_t c = cand ? gp(cand)[j] : j;
    const GLOBAL double* pv = gp(d.V) + (c / PBM) * d.vld * PBM + c % PBM;
    double vv = 0.0;
    // (32 loads in flight per thread: the chain of multiply-adds is the order, the loads are free)
#pragma unroll 32
    for (int64_t n = 0; n < d.N; ++n) {
      const double v = pv[n * PBM];
      vv = __builtin_fma(v, v, vv);
    }
    const CovPt p = cov_pt(h, d.grid, c);
    dc = (cov_entry(h, p, p, vv) + h.noiseH) + h.jitter;
  }
  for (int k = 0; k < nw; ++k) {
    double val = -__builtin_inf();
    if (ok) {
      double sum = 0.0;
      for (int sg = 0; sg < nseg; ++sg) sum = sum + gp(partial)[((int64_t)sg * nw + k) * nc + j];
      val = div_(sum, dc);
      gp(out)[k * ldo + j] = val;
    }
    double bv = val;
    int64_t bi = ok ? j : INT64_MAX;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) argmax_pair(bv, bi, __shfl_xor(bv, off), __shfl_xor(bi, off));
    if (lane == 0) {
      rv[wv] = bv;
      ri[wv] = bi;
    }
    __syncthreads();
    if (tid == 0) {
      for (int ww = 1; ww < 4; ++ww) argmax_pair(bv, bi, rv[ww], ri[ww]);
      gp(bval)[(int64_t)k * gridDim.x + blockIdx.x] = bv;
      gp(bpos)[(int64_t)k * gridDim.x + blockIdx.x] = bi;
    }
    __syncthreads();
  }
}

// best[k], best_pos[k] = argmax_pair over bval / bpos [k][0, nblk); one workgroup per k
__global__ __launch_bounds__(NT) void k_ivr_best(const double* __restrict__ bval, const int64_t* __restrict__ bpos,
                                                 int64_t nblk, double* __restrict__ best,
                                                 int64_t* __restrict__ best_pos) {
  __shared__ double rv[4];
  __shared__ int64_t ri[4];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int k = blockIdx.x;
  double bv = -__builtin_inf();
  int64_t bi = INT64_MAX;
  for (int64_t b = tid; b < nblk; b += NT) argmax_pair(bv, bi, gp(bval)[k * nblk + b], gp(bpos)[k * nblk + b]);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) argmax_pair(bv, bi, __shfl_xor(bv, off), __shfl_xor(bi, off));
  if (lane == 0) {
    rv[wv] = bv;
    ri[wv] = bi;
  }
  __syncthreads();
  if (tid == 0) {
    for (int ww = 1; ww < 4; ++ww) argmax_pair(bv, bi, rv[ww], ri[ww]);
    gp(best)[k] = bv;
    gp(best_pos)[k] = bi;
  }
}

hipError_t launch_ivr_partial(const GPDesc& d, const int64_t* cand, int64_t nc, const double* w, int nw, int64_t ldw,
                              double* partial, hipStream_t s) {
  if (nc <= 0) return hipSuccess;
  const dim3 grid((unsigned)((nc + 63) / 64), (unsigned)ivr_segments(d.M));
  hipLaunchKernelGGL(k_ivr_partial, grid, dim3(NT), 0, s, d, cand, nc, w, nw, ldw, partial);
  return hipGetLastError();
}

hipError_t launch_ivr(const GPDesc& d, const int64_t* cand, int64_t nc, const double* w, int nw, int64_t ldw,
                      double* partial, double* out, int64_t ldo, double* bval, int64_t* bpos, double* best,
                      int64_t* best_pos, hipStream_t s) {
  if (nc <= 0) return hipSuccess;
  const int nseg = (int)ivr_segments(d.M);
  hipError_t e = launch_ivr_partial(d, cand, nc, w, nw, ldw, partial, s);
  if (e != hipSuccess) return e;
  const int64_t nblk = ivr_finish_blocks(nc);
  hipLaunchKernelGGL(k_ivr_finish, dim3((unsigned)nblk), dim3(NT), 0, s, d, cand, nc, partial, nseg, nw, out, ldo,
                     bval, bpos);
  e = hipGetLastError();
  if (e != hipSuccess || !best) return e;
  hipLaunchKernelGGL(k_ivr_best, dim3((unsigned)nw), dim3(NT), 0, s, bval, bpos, nblk, best, best_pos);
  return hipGetLastError();
}

}  // namespace mfgp
