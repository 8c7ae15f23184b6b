// Products of the posterior covariance with grid vectors from the resident V, and the
// kernels of the greedy integrated-variance planner on top of them, for gfx950
// (MI355X), fp64.
//
// The posterior covariance on the grid's M cells is C = K** - V^T V with the resident
// V = L^-1 psi^T ([tile][row][64 cells], mfgp_cov.h), so for a grid vector x
//   u = C x = K** x - V^T (V x)
// is two streamed passes over V and the M x M matrix never exists:
//
//   k_cov_dot    pass A, p = V x. One workgroup per (cell segment, chunk of COV_RC
//                training rows). A segment is COV_SEG consecutive 64-cell tiles, so the
//                partition of the cells depends on M alone. The workgroup stores
//                partial[segment][n] for its rows; rows >= N and cells >= M contribute
//                zeros and are never loaded.
//   k_cov_psum   p[n] = the segments' partials added in segment order from 0.0.
//   k_kss_axes,  the separable form of K** x for a lattice grid (cell ix sx + iy sy holds
//   k_kss_t,     (xax[ix], yax[iy])): k** factorises over the axes for each kernel part,
//   k_kss_out    s kx(ix, ix') ky(iy, iy') (MF: rho^2 s_L k_L + s_H k_H), so K** x is
//                sum_part s_part Kx X Ky^T on the nx x ny reshaping of x: the axis Gram
//                matrices once per call, then two small products per part.
//   k_cov_apply  pass B, u(c) = (K** x)(c) - sum_n V[n,c] p[n]. One workgroup per tile.
//                K** x is k_kss_out's, or (the general form, any grid) sum_j k**(c, j) x_j
//                with cov_pt / cov_entry(.., 0.0) evaluated on the fly: M^2 exps. The
//                stand-alone form stores u; the planner's form updates the numerators S.
//
// The planner (plan_ivr_run in mfgp_planners.hip: one loop behind mfgp_batch_plan_ivr and,
// as its batch of one, mfgp_plan_ivr). For one member, with weights w, C_t the covariance
// after t picks and S_t(c) = sum_i w_i C_t(i,c)^2, picking c* as a hifi row gives
// C_{t+1} = C_t - g g^T, g(i) = C_t(i,c*) / sqrt(C_t(c*,c*) + sigma_H + jitter): the row
// the one-row bordered append stores as row N + t of V. With x = w o g, tau = sum_i w_i g_i^2
// and u = C_{t+1} x (both passes over the t + 1 appended rows too):
//   S_{t+1}(c) = S_t(c) - 2 g(c) u(c) - g(c)^2 tau
//   score_{t+1}(c) = S_{t+1}(c) / (var_{t+1}(c) + sigma_H + jitter)
//
//   k_ivr_pick_batch  one workgroup per member: the argmax of the score over the allowed
//                positions of its list (argmax_pair's rule; a position of an exhausted
//                group -- a per-member array of group counters against the quotas -- is
//                masked), the chosen cell's coordinates and posterior mean as the next
//                hifi row, (cell, position, gain) recorded, the device gate closed at the
//                end of the run (as k_choi_select).
//   k_plan_x_batch  after the step: g = row N + t of V, x = w o g, tau's partial sums.
//   k_plan_scatter  S from k_ivr_partial's numerators over the member's list: the segments
//                in order, undivided, stored at the candidates' cells only.
// Every kernel of the loop is a no-op once the gate is closed. No atomics, no flags, no
// cross-workgroup hand-offs, no calls: everything meets at launch boundaries.
//
// The loop's kernels are the batched forms (k_ivr_pick_batch, k_plan_x_batch,
// k_cov_dot_batch, k_cov_psum_batch, k_kss_t_batch, k_kss_out_batch, k_cov_apply_batch):
// they serve every member of a batch of models with one launch each per pick. The member
// is the slowest grid dimension; its arguments (PlanMember) sit in a device array the
// workgroup reads uniformly, with the member's row count before the run, so the array
// serves a chunk of iterations and the iteration's index is the only argument that
// changes. The grids are the largest member's, and a workgroup past its own member's
// cells or rows exits. The covariance product's kernels also have by-value forms
// (k_cov_dot, k_cov_psum, k_kss_t, k_kss_out, k_cov_apply: mfgp_cov_apply's); each pair
// calls one __forceinline__ body, so a member's order of sums is the stand-alone
// product's and depends on its own M alone.
//
// Order of sums. Pass A: thread (wave wv, lane) owns the cell pair lane & 31 of every tile
// of the segment and the rows 8 k + 2 wv + (lane >> 5) of the chunk; for a row it adds the
// tiles' products in tile order (one fused multiply-add chain per cell of the pair), adds
// the pair's two sums, and the 32 lanes' values meet in a butterfly (xor 16, 8, 4, 2, 1).
// Pass B: thread (wv, lane) owns the same cell pair and the rows n = 8 k + 2 wv + (lane >> 5),
// k ascending, one fused multiply-add chain per cell; a cell's eight row-group sums are
// added as group 0, 1, .. 7 starting from the first. The general K** x is split the same
// way over j = 8 k + group. The separable sums run over the axis index ascending, part L
// then part H. tau: 256 cells per partial, a fixed tree, the partials added in order from
// 0.0. None of it depends on the number of columns of a call or on their order.
#include <hip/hip_runtime.h>

#include "mfgp_cov.h"

namespace mfgp {

__device__ __forceinline__ bool gate_closed(const int* gate) { return gate && *gp(gate) == 0; }

// the cell pair at p: nv = 2 both cells (one 16-byte load), 1 the first only, 0 neither
__device__ __forceinline__ dv2 ld_pair(const GLOBAL double* p, int nv) {
  if (nv == 2) return *reinterpret_cast<const GLOBAL dv2*>(p);
  dv2 r = {0.0, 0.0};
  if (nv == 1) r.x = p[0];
  return r;
}
__device__ __forceinline__ int pair_cells(int64_t c0, int64_t M) {
  return c0 + 1 < M ? 2 : (c0 < M ? 1 : 0);
}

// ---- pass A -------------------------------------------------------------------------------
constexpr int COV_U = 4;   // rows in flight per thread (each COV_SEG 16-byte loads)

// workgroup (bx: cell segment, by: chunk of rows) of pass A
__device__ __forceinline__ void cov_dot_body(const CovApply& a, unsigned bx, unsigned by) {
  if (gate_closed(a.gate)) return;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int hh = lane >> 5, cp = lane & 31;
  const int64_t t0 = (int64_t)bx * COV_SEG;
  const int64_t r0 = (int64_t)by * COV_RC;
  dv2 xs[COV_SEG];
  int nv[COV_SEG];
#pragma unroll
  for (int t = 0; t < COV_SEG; ++t) {
    const int64_t c0 = (t0 + t) * PBM + 2 * cp;
    nv[t] = pair_cells(c0, a.M);
    xs[t] = ld_pair(gp(a.x) + c0, nv[t]);
  }
  const GLOBAL double* base = gp(a.V) + t0 * a.vld * PBM + 2 * cp;
  for (int k0 = 0; k0 < COV_RC / 8; k0 += COV_U) {
    dv2 v[COV_U][COV_SEG];
#pragma unroll
    for (int u = 0; u < COV_U; ++u) {
      const int64_t n = r0 + 8 * (k0 + u) + 2 * wv + hh;
#pragma unroll
      for (int t = 0; t < COV_SEG; ++t)
        v[u][t] = ld_pair(base + ((int64_t)t * a.vld + n) * PBM, n < a.N ? nv[t] : 0);
    }
#pragma unroll
    for (int u = 0; u < COV_U; ++u) {
      const int64_t n = r0 + 8 * (k0 + u) + 2 * wv + hh;
      double sx = 0.0, sy = 0.0;
#pragma unroll
      for (int t = 0; t < COV_SEG; ++t) {
        sx = __builtin_fma(v[u][t].x, xs[t].x, sx);
        sy = __builtin_fma(v[u][t].y, xs[t].y, sy);
      }
      double r = sx + sy;
#pragma unroll
      for (int off = 16; off > 0; off >>= 1) r = r + __shfl_xor(r, off);
      if (cp == 0 && n < a.N) gp(a.part)[(int64_t)bx * a.pld + n] = r;
    }
  }
}

__global__ __launch_bounds__(NT) void k_cov_dot(const CovApply a) { cov_dot_body(a, blockIdx.x, blockIdx.y); }

// The planner's forms (plan_ivr_run): member blockIdx.z of the device array ms, its
// product's arguments with the rows appended up to iteration `it`. The grids are the
// largest member's: a workgroup past its own member's cells or rows exits.
__device__ __forceinline__ CovApply member_apply(const PlanMember& m, int64_t it) {
  CovApply a = m.a;
  a.N += it + 1;
  return a;
}

__global__ __launch_bounds__(NT) void k_cov_dot_batch(const PlanMember* __restrict__ ms, int64_t it) {
  const PlanMember& m = ms[blockIdx.z];
  const CovApply a = member_apply(m, it);
  if ((int)blockIdx.x >= m.nseg || (int64_t)blockIdx.y * COV_RC >= a.N) return;
  cov_dot_body(a, blockIdx.x, blockIdx.y);
}

__device__ __forceinline__ void cov_psum_body(const CovApply& a, int nseg, unsigned bx) {
  if (gate_closed(a.gate)) return;
  const int64_t n = (int64_t)bx * NT + threadIdx.x;
  if (n >= a.N) return;
  double s = 0.0;
  for (int sg = 0; sg < nseg; ++sg) s = s + gp(a.part)[(int64_t)sg * a.pld + n];
  gp(a.p)[n] = s;
}

__global__ __launch_bounds__(NT) void k_cov_psum(const CovApply a, int nseg) { cov_psum_body(a, nseg, blockIdx.x); }

__global__ __launch_bounds__(NT) void k_cov_psum_batch(const PlanMember* __restrict__ ms, int64_t it) {
  const PlanMember& m = ms[blockIdx.y];
  cov_psum_body(member_apply(m, it), m.nseg, blockIdx.x);
}

// ---- the separable K** x ---------------------------------------------------------------------
// unit-scale axis Gram entry exp(-(a_i / l - a_j / l)^2 / 2), se_scaled's operations on one axis
__device__ __forceinline__ double axis_k(double ai, double aj, double l) {
#pragma clang fp contract(off)
  const double dx = div_(ai, l) - div_(aj, l);
  return exp(-0.5 * (dx * dx));
}

// ax [parts][nx][nx] | ay [parts][ny][ny] (KssArgs): one thread per entry
__global__ __launch_bounds__(NT) void k_kss_axes(const KssArgs k) {
  const int64_t nx2 = (int64_t)k.nx * k.nx, ny2 = (int64_t)k.ny * k.ny;
  const int64_t e = (int64_t)blockIdx.x * NT + threadIdx.x;
  const int64_t per = nx2 + ny2;
  if (e >= per * k.parts) return;
  const int part = (int)(e / per);
  const int64_t r = e % per;
  const double l = part ? k.h.lH : k.h.lL;
  if (r < nx2) {
    const int64_t i = r / k.nx, j = r % k.nx;
    gp(k.ax)[part * nx2 + r] = axis_k(gp(k.grid)[2 * (i * k.sx)], gp(k.grid)[2 * (j * k.sx)], l);
  } else {
    const int64_t q = r - nx2, i = q / k.ny, j = q % k.ny;
    gp(k.ay)[part * ny2 + q] = axis_k(gp(k.grid)[2 * (i * k.sy) + 1], gp(k.grid)[2 * (j * k.sy) + 1], l);
  }
}

// T[part][ix][iy] = sum_iy' Ky_part[iy][iy'] x(ix, iy'), iy' ascending
__device__ __forceinline__ void kss_t_body(const KssArgs& k, const double* __restrict__ x, double* __restrict__ T,
                                           const int* gate, unsigned bx) {
  if (gate_closed(gate)) return;
  const int64_t Mc = (int64_t)k.nx * k.ny;
  const int64_t e = (int64_t)bx * NT + threadIdx.x;
  if (e >= Mc * k.parts) return;
  const int part = (int)(e / Mc);
  const int64_t r = e % Mc, ix = r / k.ny, iy = r % k.ny;
  const GLOBAL double* ky = gp(k.ay) + ((int64_t)part * k.ny + iy) * k.ny;
  const GLOBAL double* xr = gp(x) + ix * k.sx;
  double s = 0.0;
  for (int64_t j = 0; j < k.ny; ++j) s = __builtin_fma(ky[j], xr[j * k.sy], s);
  gp(T)[e] = s;
}

__global__ __launch_bounds__(NT) void k_kss_t(const KssArgs k, const double* __restrict__ x, double* __restrict__ T,
                                              const int* gate) {
  kss_t_body(k, x, T, gate, blockIdx.x);
}

// (a member on the general K** x form has no part in either launch)
__global__ __launch_bounds__(NT) void k_kss_t_batch(const PlanMember* __restrict__ ms) {
  const PlanMember& m = ms[blockIdx.y];
  if (!m.sep) return;
  kss_t_body(m.k, m.a.x, m.T, m.a.gate, blockIdx.x);
}

// out(ix, iy) = sum_part s_part sum_ix' Kx_part[ix][ix'] T[part][ix'][iy], ix' ascending, part L then H
__device__ __forceinline__ void kss_out_body(const KssArgs& k, const double* __restrict__ T, double* __restrict__ out,
                                             const int* gate, unsigned bx) {
  if (gate_closed(gate)) return;
  const int64_t Mc = (int64_t)k.nx * k.ny;
  const int64_t e = (int64_t)bx * NT + threadIdx.x;
  if (e >= Mc) return;
  const int64_t ix = e / k.ny, iy = e % k.ny;
  double res = 0.0;
  for (int part = 0; part < k.parts; ++part) {
#pragma clang fp contract(off)
    const GLOBAL double* kx = gp(k.ax) + ((int64_t)part * k.nx + ix) * k.nx;
    const GLOBAL double* tc = gp(T) + (int64_t)part * Mc + iy;
    double s = 0.0;
    for (int64_t j = 0; j < k.nx; ++j) s = __builtin_fma(kx[j], tc[j * k.ny], s);
    const double sc = part ? k.h.sH : (k.h.kind != 0 ? k.h.rho2 * k.h.sL : k.h.sL);
    res = part ? res + sc * s : sc * s;
  }
  gp(out)[ix * k.sx + iy * k.sy] = res;
}

__global__ __launch_bounds__(NT) void k_kss_out(const KssArgs k, const double* __restrict__ T, double* __restrict__ out,
                                                const int* gate) {
  kss_out_body(k, T, out, gate, blockIdx.x);
}

__global__ __launch_bounds__(NT) void k_kss_out_batch(const PlanMember* __restrict__ ms) {
  const PlanMember& m = ms[blockIdx.y];
  if (!m.sep) return;
  kss_out_body(m.k, m.T, m.kxo, m.a.gate, blockIdx.x);
}

// ---- pass B -------------------------------------------------------------------------------
constexpr int COVB_U = 8;   // rows in flight per thread

// workgroup of tile t; red: the workgroup's LDS [2][8][PBM]
__device__ __forceinline__ void cov_apply_body(const CovApply& a, int64_t t, double (*red)[8][PBM]) {
  if (gate_closed(a.gate)) return;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int hh = lane >> 5, cp = lane & 31, rg = 2 * wv + hh;
  const int64_t c0 = t * PBM + 2 * cp;
  const int nv = pair_cells(c0, a.M);
  const GLOBAL double* pv = gp(a.V) + t * a.vld * PBM + 2 * cp;
  double sx = 0.0, sy = 0.0;
  int64_t n = rg;
  for (; n + 8 * (COVB_U - 1) < a.N; n += 8 * COVB_U) {
    dv2 v[COVB_U];
    double pn[COVB_U];
#pragma unroll
    for (int u = 0; u < COVB_U; ++u) {
      v[u] = ld_pair(pv + (n + 8 * u) * PBM, nv);
      pn[u] = gp(a.p)[n + 8 * u];
    }
#pragma unroll
    for (int u = 0; u < COVB_U; ++u) {
      sx = __builtin_fma(v[u].x, pn[u], sx);
      sy = __builtin_fma(v[u].y, pn[u], sy);
    }
  }
  for (; n < a.N; n += 8) {
    const dv2 v = ld_pair(pv + n * PBM, nv);
    const double pn = gp(a.p)[n];
    sx = __builtin_fma(v.x, pn, sx);
    sy = __builtin_fma(v.y, pn, sy);
  }
  red[0][rg][2 * cp] = sx;
  red[0][rg][2 * cp + 1] = sy;
  if (!a.kx) {
    // the general K** x: this thread's share j = 8 k + rg of the sum for its two cells
    const Hyp& h = a.h;
    const CovPt pa = cov_pt(h, a.grid, nv > 0 ? c0 : 0), pb = cov_pt(h, a.grid, nv > 1 ? c0 + 1 : 0);
    double kx0 = 0.0, kx1 = 0.0;
    for (int64_t j = rg; j < a.M; j += 8) {
      const double xj = gp(a.x)[j];
      if (xj == 0.0) continue;
      const CovPt pj = cov_pt(h, a.grid, j);
      kx0 = __builtin_fma(cov_entry(h, pa, pj, 0.0), xj, kx0);
      kx1 = __builtin_fma(cov_entry(h, pb, pj, 0.0), xj, kx1);
    }
    red[1][rg][2 * cp] = kx0;
    red[1][rg][2 * cp + 1] = kx1;
  }
  __syncthreads();
  const int64_t c = t * PBM + tid;
  if (tid < PBM && c < a.M) {
#pragma clang fp contract(off)
    double vv = red[0][0][tid];
#pragma unroll
    for (int g = 1; g < 8; ++g) vv = vv + red[0][g][tid];
    double kx;
    if (a.kx) {
      kx = gp(a.kx)[c];
    } else {
      kx = red[1][0][tid];
#pragma unroll
      for (int g = 1; g < 8; ++g) kx = kx + red[1][g][tid];
    }
    const double u = kx - vv;
    if (a.u) gp(a.u)[c] = u;
    if (a.S) {
      double tau = 0.0;
      for (int i = 0; i < a.ntau; ++i) tau = tau + gp(a.tau_part)[i];
      const double g = gp(a.g)[c];
      gp(a.S)[c] = (gp(a.S)[c] - (2.0 * g) * u) - (g * g) * tau;
    }
  }
}

__global__ __launch_bounds__(NT) void k_cov_apply(const CovApply a) {
  __shared__ double red[2][8][PBM];
  cov_apply_body(a, blockIdx.x, red);
}

__global__ __launch_bounds__(NT) void k_cov_apply_batch(const PlanMember* __restrict__ ms, int64_t it) {
  __shared__ double red[2][8][PBM];
  const PlanMember& m = ms[blockIdx.y];
  if ((int64_t)blockIdx.x * PBM >= m.a.M) return;
  cov_apply_body(member_apply(m, it), blockIdx.x, red);
}

// ---- the planner's kernels -------------------------------------------------------------------
// g = row `row` of V, x = w o g, tau_part[workgroup] = sum over its 256 cells of w g^2
__device__ __forceinline__ void plan_x_body(const double* __restrict__ V, int64_t vld, int64_t row, int64_t M,
                                            const double* __restrict__ w, double* __restrict__ g,
                                            double* __restrict__ x, double* __restrict__ tau_part, const int* gate,
                                            unsigned bx, double* red) {
  if (gate_closed(gate)) return;
  const int tid = threadIdx.x;
  const int64_t c = (int64_t)bx * NT + tid;
  double tw = 0.0;
  if (c < M) {
#pragma clang fp contract(off)
    const double gv = gp(V)[((c / PBM) * vld + row) * PBM + c % PBM];
    const double wc = w ? gp(w)[c] : 1.0;
    const double xc = wc * gv;
    gp(g)[c] = gv;
    gp(x)[c] = xc;
    tw = xc * gv;
  }
  red[tid] = tw;
  __syncthreads();
  for (int s = NT / 2; s > 0; s >>= 1) {
    if (tid < s) red[tid] = red[tid] + red[tid + s];
    __syncthreads();
  }
  if (tid == 0) gp(tau_part)[bx] = red[0];
}

// (the row iteration `it` appended: a.N + it)
__global__ __launch_bounds__(NT) void k_plan_x_batch(const PlanMember* __restrict__ ms, int64_t it) {
  __shared__ double red[NT];
  const PlanMember& m = ms[blockIdx.y];
  const CovApply& a = m.a;
  if ((int64_t)blockIdx.x * NT >= a.M) return;
  plan_x_body(a.V, a.vld, a.N + it, a.M, m.w, const_cast<double*>(a.g), const_cast<double*>(a.x),
              const_cast<double*>(a.tau_part), a.gate, blockIdx.x, red);
}

// S[cand[j]] (cand null: S[j]) = k_ivr_partial's numerators partial[segment][j] (nw = 1, j < nc)
// added in segment order. A cell listed twice receives the same bits twice.
__device__ __forceinline__ void plan_ssum_body(const double* __restrict__ partial, int nseg, int64_t nc,
                                               const int64_t* __restrict__ cand, double* __restrict__ S) {
  const int64_t j = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (j >= nc) return;
  double s = 0.0;
  for (int sg = 0; sg < nseg; ++sg) s = s + gp(partial)[(int64_t)sg * nc + j];
  gp(S)[cand ? gp(cand)[j] : j] = s;
}

__global__ __launch_bounds__(NT) void k_plan_scatter(const double* __restrict__ partial, int nseg, int64_t nc,
                                                     const int64_t* __restrict__ cand, double* __restrict__ S) {
  plan_ssum_body(partial, nseg, nc, cand, S);
}

// One workgroup's pick for one model. q.group set: position j is
// allowed while its group has made fewer picks than its quota.
__device__ __forceinline__ void ivr_pick_body(const PlanPick& q, double* rv, int64_t* ri) {
  int* gate = reinterpret_cast<int*>(q.state);
  if (*gp(gate) == 0) return;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int64_t cnt = gp(q.state)[1];
  if (*gp(q.status) != INT_MAX || cnt >= q.n_points) {
    if (tid == 0) *gp(gate) = 0;
    return;
  }
  double bv = -__builtin_inf();
  int64_t bi = INT64_MAX;
  for (int64_t j = tid; j < q.nc; j += NT) {
#pragma clang fp contract(off)
    if (q.group) {
      const int gj = gp(q.group)[j];
      if (gp(q.gcount)[gj] >= (q.quota ? gp(q.quota)[gj] : 1)) continue;
    }
    const int64_t c = q.cand ? gp(q.cand)[j] : j;
    const double dc = (gp(q.var)[c] + q.noise) + q.jitter;
    argmax_pair(bv, bi, div_(gp(q.S)[c], dc), j);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) argmax_pair(bv, bi, __shfl_xor(bv, off), __shfl_xor(bi, off));
  if (lane == 0) {
    rv[wv] = bv;
    ri[wv] = bi;
  }
  __syncthreads();
  if (tid != 0) return;
  for (int ww = 1; ww < 4; ++ww) argmax_pair(bv, bi, rv[ww], ri[ww]);
  if (bi < 0 || bi >= q.nc || !(bv >= q.min_gain)) {
    *gp(gate) = 0;
    return;
  }
  const int64_t c = q.cand ? gp(q.cand)[bi] : bi;
  const double gx = gp(q.grid)[2 * c], gy = gp(q.grid)[2 * c + 1];
  gp(q.xn)[0] = gx;
  gp(q.xn)[1] = gy;
  gp(q.yn)[0] = gp(q.mu)[c];
  gp(q.cells)[cnt] = c;
  gp(q.gains)[cnt] = bv;
  gp(q.pts)[2 * cnt] = gx;
  gp(q.pts)[2 * cnt + 1] = gy;
  if (q.pos) gp(q.pos)[cnt] = bi;
  if (q.group) {
    const int gb = gp(q.group)[bi];
    gp(q.gcount)[gb] = gp(q.gcount)[gb] + 1;
  }
  gp(q.state)[1] = cnt + 1;
}

// one workgroup per member
__global__ __launch_bounds__(NT) void k_ivr_pick_batch(const PlanMember* __restrict__ ms) {
  __shared__ double rv[4];
  __shared__ int64_t ri[4];
  ivr_pick_body(ms[blockIdx.x].q, rv, ri);
}

// ---- launchers -----------------------------------------------------------------------------------
static hipError_t last() { return hipGetLastError(); }

hipError_t launch_kss_axes(const KssArgs& k, hipStream_t s) {
  const int64_t n = ((int64_t)k.nx * k.nx + (int64_t)k.ny * k.ny) * k.parts;
  hipLaunchKernelGGL(k_kss_axes, dim3((unsigned)((n + NT - 1) / NT)), dim3(NT), 0, s, k);
  return last();
}

hipError_t launch_kss(const KssArgs& k, const double* x, double* T, double* out, const int* gate, hipStream_t s) {
  const int64_t Mc = (int64_t)k.nx * k.ny;
  hipLaunchKernelGGL(k_kss_t, dim3((unsigned)((Mc * k.parts + NT - 1) / NT)), dim3(NT), 0, s, k, x, T, gate);
  hipError_t e = last();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_kss_out, dim3((unsigned)((Mc + NT - 1) / NT)), dim3(NT), 0, s, k, T, out, gate);
  return last();
}

hipError_t launch_cov_apply(const CovApply& a, hipStream_t s) {
  if (a.M <= 0) return hipSuccess;
  const int nseg = (int)cov_segments(a.M);
  if (a.N > 0) {
    hipLaunchKernelGGL(k_cov_dot, dim3((unsigned)nseg, (unsigned)((a.N + COV_RC - 1) / COV_RC)), dim3(NT), 0, s, a);
    hipError_t e = last();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_cov_psum, dim3((unsigned)((a.N + NT - 1) / NT)), dim3(NT), 0, s, a, nseg);
    if ((e = last()) != hipSuccess) return e;
  }
  hipLaunchKernelGGL(k_cov_apply, dim3((unsigned)ntiles_grid(a.M)), dim3(NT), 0, s, a);
  return last();
}

hipError_t launch_plan_scatter(const double* partial, int nseg, int64_t nc, const int64_t* cand, double* S,
                               hipStream_t s) {
  if (nc <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_plan_scatter, dim3((unsigned)((nc + NT - 1) / NT)), dim3(NT), 0, s, partial, nseg, nc, cand, S);
  return last();
}

hipError_t launch_ivr_pick_batch(const PlanMember* ms, int count, hipStream_t s) {
  hipLaunchKernelGGL(k_ivr_pick_batch, dim3((unsigned)count), dim3(NT), 0, s, ms);
  return last();
}

hipError_t launch_plan_update_batch(const PlanMember* ms, int count, int64_t it, int64_t maxM, int64_t maxN,
                                    bool any_sep, hipStream_t s) {
  const unsigned B = (unsigned)count, wgM = (unsigned)((maxM + NT - 1) / NT);
  hipError_t e;
  hipLaunchKernelGGL(k_plan_x_batch, dim3((unsigned)plan_tau_parts(maxM), B), dim3(NT), 0, s, ms, it);
  if ((e = last()) != hipSuccess) return e;
  hipLaunchKernelGGL(k_cov_dot_batch, dim3((unsigned)cov_segments(maxM), (unsigned)((maxN + COV_RC - 1) / COV_RC), B),
                     dim3(NT), 0, s, ms, it);
  if ((e = last()) != hipSuccess) return e;
  hipLaunchKernelGGL(k_cov_psum_batch, dim3((unsigned)((maxN + NT - 1) / NT), B), dim3(NT), 0, s, ms, it);
  if ((e = last()) != hipSuccess) return e;
  if (any_sep) {
    hipLaunchKernelGGL(k_kss_t_batch, dim3(2 * wgM, B), dim3(NT), 0, s, ms);   // (up to two parts)
    if ((e = last()) != hipSuccess) return e;
    hipLaunchKernelGGL(k_kss_out_batch, dim3(wgM, B), dim3(NT), 0, s, ms);
    if ((e = last()) != hipSuccess) return e;
  }
  hipLaunchKernelGGL(k_cov_apply_batch, dim3((unsigned)ntiles_grid(maxM), B), dim3(NT), 0, s, ms, it);
  return last();
}

}  // namespace mfgp
