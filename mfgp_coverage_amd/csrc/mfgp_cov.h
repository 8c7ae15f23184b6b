// The operand staging and the epilogue forms of the covariance GEMM over the
// resident V, shared by k_cov_block (mfgp_cov.hip) and k_ivr_partial (mfgp_ivr.hip):
// both run the same K loop (chunks of 64 training rows, n ascending, no split-K)
// and form the same cov(i, j) = k**(i, j) - sum_n V[n,i] V[n,j], bit for bit.
#pragma once
#include <hip/hip_runtime.h>

#include "mfgp_device.h"
#include "mfgp_internal.h"

namespace mfgp {

constexpr int CKC = NB;            // training rows per K chunk (tile_mma's depth)
constexpr int CPT = CKC * 64 / NT; // panel elements per thread and chunk (16)

// One chunk of both operand panels in registers (issue-early / write-late): the
// loads of chunk c + 1 are in flight while the MFMAs of chunk c run.
struct CovStage {
  double a[CPT], b[CPT];
};

// Thread (wave w, lane) stages cell `lane` of either panel, rows n0 + 4 p + w.
// pa / pb: the cell's column of V (row n at [n * 64]); rows >= N and cells past
// the lists are zeros and are never loaded (V's rows past N may hold an older
// model's values, its tiles' cells past M nothing).
__device__ __forceinline__ void cov_fetch(CovStage& st, const GLOBAL double* pa, const GLOBAL double* pb,
                                          bool oka, bool okb, int64_t n0, int64_t N, int w) {
#pragma unroll
  for (int p = 0; p < CPT; ++p) {
    const int64_t n = n0 + 4 * p + w;
    const bool in = n < N;
    st.a[p] = (in && oka) ? pa[n * PBM] : 0.0;
    st.b[p] = (in && okb) ? pb[n * PBM] : 0.0;
  }
}

// As[swz(k, i)] = V[n0 + k][row cell i], Bs[swz(k, j)] = V[n0 + k][column cell j]
__device__ __forceinline__ void cov_put(double* __restrict__ As, double* __restrict__ Bs, const CovStage& st,
                                        int w, int lane) {
#pragma unroll
  for (int p = 0; p < CPT; ++p) {
    const int k = 4 * p + w;
    As[swz(k, lane)] = st.a[p];
    Bs[swz(k, lane)] = st.b[p];
  }
}

// A cell's coordinates over both length scales (x / l, as the reference scales
// before it subtracts, gp:77-78).
struct CovPt {
  double xL, yL, xH, yH;
};
__device__ __forceinline__ CovPt cov_pt(const Hyp& h, const double* __restrict__ grid, int64_t cell) {
  const double x = gp(grid)[2 * cell], y = gp(grid)[2 * cell + 1];
  CovPt p;
  p.xL = div_(x, h.lL);
  p.yL = div_(y, h.lL);
  p.xH = div_(x, h.lH);
  p.yH = div_(y, h.lH);
  return p;
}

// k**(x_i, x_j) (gp:146 SF: s k; gp:435-436 MF: rho^2 s_L k_L + s_H k_H) minus the
// accumulated V_i . V_j, no FMA contraction.
__device__ __forceinline__ double cov_entry(const Hyp& h, const CovPt& a, const CovPt& b, double vv) {
#pragma clang fp contract(off)
  const double kl = se_scaled(a.xL, a.yL, b.xL, b.yL, h.sL);
  double kss = kl;
  if (h.kind != 0) {
    const double kh = se_scaled(a.xH, a.yH, b.xH, b.yH, h.sH);
    kss = h.rho2 * kl + kh;
  }
  return kss - vv;
}

}  // namespace mfgp
