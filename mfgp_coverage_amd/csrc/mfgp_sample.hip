// Pathwise (Matheron) samples of the prior and the posterior on a lattice grid for
// gfx950 (MI355X), fp64.
//
// A posterior sample is a prior sample corrected through the data:
//   f_post(grid) = m_H + f_prior(grid) + psi K^-1 (y - m - f_prior(X) - eps)
//                = m_H + f_prior(grid) + V^T (L^-1 r),   V = L^-1 psi^T resident,
//   r = (y - m) - f_prior(X) - sqrt(noise_fid + jitter) eps.
// The SE kernel separates over the lattice's two axes, so with the axis factors
// Ax Ax^T = Kx, Ay Ay^T = Ky (pivoted Cholesky on the host, n x r each) the field
// sqrt(s) Ax Z Ay^T has exactly the prior covariance; an MF model has two independent
// fields u_L (s_L, l_L) and delta (s_H, l_H), hifi = rho u_L + delta, lofi = u_L.
// Per chunk of at most 64 samples, consecutive launches on the context's stream:
//   k_sample_t       T = Ax Z per sample and field                      (plain FMA)
//   k_sample_field   out = mean + sum_f c_f T Ay^T over the grid's cells  (plain FMA)
//   k_sample_resid   R[n][s] = r of training row n, sample s, from T at the row's cell
//   k_sample_solve   W = L^-1 R: the blocked forward substitution of k_predict /
//                    look_subst (mfgp_look.hip) with the right-hand sides loaded where
//                    those generate psi; one workgroup, Linv's diagonal-block inverses
//                    and the LDS-DMA ring of mfgp_device.h
//   k_sample_gemm    out[s][cells] += sum_n V[tile][n][cell] W[n][s]: one workgroup per
//                    64-cell V tile and 64 samples, f64 MFMA, V read once per chunk
// No flags, atomics or cross-workgroup hand-offs. Every reduction runs in a fixed
// order per column and a column's operands are its own sample's alone, so a sample's
// bits depend only on its normals: not on S, its position or the other samples.
#include <hip/hip_runtime.h>

#include "mfgp_device.h"
#include "mfgp_internal.h"

namespace mfgp {

// u_f at lattice cell (ix, iy) of sample s: sum_b T[s][f][ix][b] AyT[f][b][iy], b ascending.
__device__ __forceinline__ double sample_u(const SampleArgs& a, int f, int s, int ix, int iy) {
  const GLOBAL double* t = gp(a.T) + (((int64_t)s * a.fields + f) * a.nx + ix) * a.tw;
  const GLOBAL double* ay = gp(a.AyT[f]) + iy;
  double u = 0.0;
  for (int b = 0; b < a.ry[f]; ++b) u = fma(t[b], ay[(int64_t)b * a.ny], u);
  return u;
}

// T[s][f][ix][b] = sum_a Ax[f][ix][a] Z[s][f][a][b], a ascending. Grid (.., fields, Sc).
__global__ __launch_bounds__(NT) void k_sample_t(const SampleArgs a) {
  const int f = blockIdx.y, s = blockIdx.z;
  const int rx = a.rx[f], ry = a.ry[f];
  const int64_t e = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (e >= (int64_t)a.nx * ry) return;
  const int ix = (int)(e / ry), b = (int)(e % ry);
  const GLOBAL double* z = gp(a.Z) + (int64_t)s * a.ldz + a.zoff[f] + b;
  const GLOBAL double* ax = gp(a.Ax[f]) + (int64_t)ix * rx;
  double t = 0.0;
  for (int k = 0; k < rx; ++k) t = fma(ax[k], z[(int64_t)k * ry], t);
  gp(a.T)[(((int64_t)s * a.fields + f) * a.nx + ix) * a.tw + b] = t;
}

// The hifi field of sample s at cell e: c0 u_0 (+ c1 u_1), SF: sqrt(s) u; MF: rho sqrt(s_L) u_L +
// sqrt(s_H) delta.
__device__ __forceinline__ double sample_hifi(const SampleArgs& a, int s, int ix, int iy) {
  double v = a.cH[0] * sample_u(a, 0, s, ix, iy);
  if (a.fields > 1) v = fma(a.cH[1], sample_u(a, 1, s, ix, iy), v);
  return v;
}

// out[s][e] = mean + hifi field. Grid (ceil(M / NT), Sc).
__global__ __launch_bounds__(NT) void k_sample_field(const SampleArgs a) {
  const int s = blockIdx.y;
  const int64_t e = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (e >= a.M) return;
  // cell e = ix sx + iy sy with (sx, sy) = (ny, 1) or (1, nx)
  const int ix = a.sy == 1 ? (int)(e / a.ny) : (int)(e % a.nx);
  const int iy = a.sy == 1 ? (int)(e % a.ny) : (int)(e / a.nx);
  gp(a.out)[(int64_t)s * a.ldo + e] = a.mean + sample_hifi(a, s, ix, iy);
}

// R[n][s] = (y_n - m_n) - f_prior(X_n) - sd_n eps[s][n] for s < Sc, zero columns beyond.
// A lofi row sees u_L at its cell, a hifi row the hifi field. Grid ceil(N 64 / NT).
__global__ __launch_bounds__(NT) void k_sample_resid(const SampleArgs a) {
  const int64_t e = (int64_t)blockIdx.x * NT + threadIdx.x;
  const int64_t n = e >> 6;
  const int s = (int)(e & 63);
  if (n >= a.N) return;
  double r = 0.0;
  if (s < a.Sc) {
    const int li = gp(a.lidx)[n];
    const int ix = li & 0xffff, iy = li >> 16;
    const bool lo = n < a.NL;
    const double fp = lo ? a.cL * sample_u(a, 0, s, ix, iy) : sample_hifi(a, s, ix, iy);
    const double eps = gp(a.Z)[(int64_t)s * a.ldz + a.zoff[2] + n];
    r = ((gp(a.y)[n] - (lo ? a.meanL : a.meanH)) - fp) - (lo ? a.sdL : a.sdH) * eps;
  }
  gp(a.R)[e] = r;
}

// W = L^-1 R for the 64 columns of R [>= N][64], rows [0, N) stored to W[row * 64 + column]:
// look_subst (mfgp_look.hip) with the block's right-hand sides loaded where it generates
// psi. lds: NSTAGE * STAGE doubles. W's rows are re-read by the ring's DMA; R is only read.
__device__ __forceinline__ void sample_subst(const SampleArgs& a, double* lds) {
  double* const img = lds;
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave id (uniform)
  const int r = lane & 15, q = lane >> 4;
  const int p16 = w * 16;   // diagonal-step rows of this wave inside a 64-row half
  const int64_t N = a.N, ld = a.ld;
  const int64_t nrb = prow_blocks(N);
  const int64_t nbf = nblocks_factor(N);
  const double* __restrict__ Amat = a.A;
  double* __restrict__ Vt = a.W;
  const __amdgpu_buffer_rsrc_t rsA = make_rsrc(Amat, (int64_t)8 * ld * ld);
  const __amdgpu_buffer_rsrc_t rsV = make_rsrc(Vt, (int64_t)8 * a.wld * PBM);
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
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int64_t g = base + w * 32 + mt * 16 + q + 4 * v;
#pragma unroll
        for (int nt = 0; nt < 4; ++nt)   // acc = -rhs + sum L W; rows >= N are never loaded
          acc.c[mt][nt][v] = g < N ? -gp(a.R)[g * PBM + nt * 16 + r] : 0.0;
      }
    double frag[16];
    if (nk > 0) {
      // (the right-hand-side loads above were issued after the prologue's DMA: wait for all)
      vm_wait_all();
      __builtin_amdgcn_s_barrier();
    }
    for (int s = 0; s < nk; ++s) {
      const double* cur = lds + (s % NSTAGE) * STAGE;
      if (s + 2 < nk) dma_step(lds + ((s + 2) % NSTAGE) * STAGE, base, (int64_t)(s + 2) * KS);
      main_mma(cur, cur + KS * PW, acc, w, lane);
      if (s + 2 < nk) asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"(GLDS_PER_STEP) : "memory");
      else asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");
    }
    // ---- diagonal block: W_I = L_II^-1 (rhs - L W), two 64-row halves ----
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
    if (has_b) load_afrag(frag, Amat + fa * NB * ld + fb * NB, ld, p16, lane);   // L_ba
#pragma unroll
    for (int nt = 0; nt < 4; ++nt)
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int row = p16 + q + 4 * v, col = nt * 16 + r;
        if (row < nin) gp(Vb)[row * PBM + col] = vh.c[nt][v];
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
          if (row < nin) gp(Vb)[row * PBM + col] = vh.c[nt][v];
        }
    }
    vm_wait_all();      // W_I stores complete before any later DMA reads them
    __syncthreads();    // and before the next prologue overwrites the LDS images
  }
}

__global__ __launch_bounds__(PNT, 2) void k_sample_solve(const SampleArgs a) {
  __shared__ double lds[NSTAGE * STAGE];
  sample_subst(a, lds);
}

// 64 rows n0 .. n0 + 63 of a [rows][64] tile in registers (issue-early / write-late);
// rows >= N are zeros and never loaded (they may hold an older call's values).
__device__ __forceinline__ void sample_fetch(TileRegs& t, const double* __restrict__ G, int64_t n0, int64_t N,
                                             int tid) {
#pragma unroll
  for (int p = 0; p < 8; ++p) {
    const int64_t n = n0 + p * 8 + (tid >> 5);
    dv2 v = {0.0, 0.0};
    if (n < N) v = *reinterpret_cast<const GLOBAL dv2*>(gp(G) + n * PBM + (tid & 31) * 2);
    t.v[p] = v;
  }
}

// out[s][c0 + j] += sum_n W[n][s] V[tile][n][j], n ascending (no split-K): accumulator
// row = sample, column = cell. Grid ceil(M / 64).
__global__ __launch_bounds__(NT, 2) void k_sample_gemm(const SampleArgs a) {
  __shared__ double As[TILE];
  __shared__ double Bs[TILE];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int wm = w >> 1, wn = w & 1;
  const int64_t c0 = (int64_t)blockIdx.x * PBM;
  const int64_t N = a.N;
  const double* __restrict__ Vt = a.V + (int64_t)blockIdx.x * a.vld * PBM;
  Acc acc;
  acc_zero(acc);
  TileRegs ta, tb;
  sample_fetch(ta, a.W, 0, N, tid);
  sample_fetch(tb, Vt, 0, N, tid);
  for (int64_t n0 = 0; n0 < N; n0 += NB) {
    tile_put_k(As, ta, tid);
    tile_put_k(Bs, tb, tid);
    __syncthreads();
    if (n0 + NB < N) {
      sample_fetch(ta, a.W, n0 + NB, N, tid);
      sample_fetch(tb, Vt, n0 + NB, N, tid);
    }
    tile_mma<false>(As, Bs, acc, wm, wn, lane);
    __syncthreads();
  }
  const int r = lane & 15, q = lane >> 4;
#pragma unroll
  for (int mt = 0; mt < 2; ++mt)
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int s = acc_row(wm, mt, q, v);
      if (s >= a.Sc) continue;
#pragma unroll
      for (int nt = 0; nt < 2; ++nt) {
        const int64_t c = c0 + acc_col(wn, nt, r);
        if (c < a.M) {
          GLOBAL double* o = gp(a.out) + (int64_t)s * a.ldo + c;
          *o = *o + acc.c[mt][nt][v];
        }
      }
    }
}

hipError_t launch_sample_prior(const SampleArgs& a, hipStream_t s) {
  if (a.Sc <= 0 || a.M <= 0) return hipSuccess;
  int64_t mt = 0;
  for (int f = 0; f < a.fields; ++f) mt = mt > (int64_t)a.nx * a.ry[f] ? mt : (int64_t)a.nx * a.ry[f];
  hipLaunchKernelGGL(k_sample_t, dim3((unsigned)((mt + NT - 1) / NT), (unsigned)a.fields, (unsigned)a.Sc), dim3(NT), 0,
                     s, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_sample_field, dim3((unsigned)((a.M + NT - 1) / NT), (unsigned)a.Sc), dim3(NT), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_sample_resid(const SampleArgs& a, hipStream_t s) {
  if (a.N <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_sample_resid, dim3((unsigned)((a.N * 64 + NT - 1) / NT)), dim3(NT), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_sample_solve(const SampleArgs& a, hipStream_t s) {
  if (a.N <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_sample_solve, dim3(1), dim3(PNT), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_sample_gemm(const SampleArgs& a, hipStream_t s) {
  if (a.N <= 0 || a.M <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_sample_gemm, dim3((unsigned)ntiles_grid(a.M)), dim3(NT), 0, s, a);
  return hipGetLastError();
}

}  // namespace mfgp
