// HIP kernels of the GP posterior update for gfx950 (MI355X), fp64.
//
// Reference path (MSU-dcypherlab/mfgp-coverage, gaussian_process.py):
//   k_assemble    <- kernel(X,X) + sigma_n I + jitter I, SF gp:253-254, MF gp:523-529
//                    (+ one augmented row r = y - m so the factor also yields z = L^-1 r)
//   k_potrf_diag  \
//   k_panel        > np.linalg.cholesky (gp:254, gp:529), blocked right-looking, NB = 64,
//   k_syrk        /  with the explicit inverse of every diagonal block kept for the solves
//   k_predict     <- predict (gp:121-148 / gp:401-438): psi = k(X*,X) generated in registers,
//                    V = L^-1 psi^T by blocked forward substitution on f64 MFMA, and the
//                    epilogue mu = m + V^T z (= m + psi alpha), var = k** - colsum(V o V)
//                    (= diag(k** - psi K^-1 psi^T)); the M x M matrices of the reference
//                    are never formed.
//
// Matrices are column-major; 64x64 operand tiles are staged "k-major" in LDS,
// As[k][i], with an XOR swizzle of bit 4 of the column on odd k so that the
// ds_read_b64 fragment loads of v_mfma_f64_16x16x4f64 are bank-conflict free.
// f64 MFMA fragment maps (pinned on the hardware by tools/probe_mfma_f64.hip):
//   A[i][k]: lane l holds A[l&15][l>>4];  B[k][j]: lane l holds B[l>>4][l&15];
//   C/D:     lane l, reg v holds C[(l>>4) + 4v][l&15].
#include <climits>
#include <cstring>
#include <type_traits>
#include "mfgp_internal.h"

// Diagnostic phase stamps (tools/bench_diag.hip builds with -DMFGP_STAMPS); no-op otherwise.
// Defined ahead of mfgp_device.h, whose factor_invert_64 stamps its phases.
#ifdef MFGP_STAMPS
namespace mfgp {
__device__ long long* g_stamps;
}
#define STAMP(id)                                                                        \
  do {                                                                                   \
    if (threadIdx.x == 0 && blockIdx.x == 0) g_stamps[id] = __builtin_amdgcn_s_memtime(); \
  } while (0)
#else
#define STAMP(id) \
  do {            \
  } while (0)
#endif
#include "mfgp_device.h"

namespace mfgp {

// k_inc_stream timeline stamps (GP 0 only; diagnostic builds)
#ifdef MFGP_STAMPS
#define FSTAMP(id)                                                                                 \
  do {                                                                                             \
    if (threadIdx.x == 0 && blockIdx.x == 0)                                                       \
      atomicMax((unsigned long long*)&g_stamps[id], (unsigned long long)__builtin_amdgcn_s_memrealtime()); \
  } while (0)
// per-workgroup k_inc_stream trace: g_stamps[64 + 8 * (linear WG id) + slot]
#define WTRACE(slot)                                                                                 \
  do {                                                                                               \
    if (threadIdx.x == 0) {                                                                          \
      long long* wt_ = g_stamps + 64 + 8 * (blockIdx.y * gridDim.x + blockIdx.x);                     \
      wt_[slot] = __builtin_amdgcn_s_memrealtime();                                                  \
      if ((slot) == 0)                                                                               \
        wt_[7] = ((long long)__builtin_amdgcn_s_getreg(20 | (31 << 11)) << 32) |                       \
                 (unsigned)__builtin_amdgcn_s_getreg(4 | (31 << 11));                                \
    }                                                                                                \
  } while (0)
// the lattice step's second launch (k_lat_gemm2/3): its workgroups at role 1024 + tile.
// k_lat_gemm2's slots: 0 start / 1 first ring stage landed / 2 K loop done / 3 the
// splits' sums stored (barrier) / 6 cells computed / 4 end (thread 0 stamps: the tile's
// arrival, on the last wave where it goes ahead of the stores, has no stamp)
#define WTRACE2(slot)                                                                               \
  do {                                                                                               \
    if (threadIdx.x == 0) {                                                                          \
      long long* wt_ = g_stamps + 64 + 8 * ((1024 + blockIdx.y) * gridDim.x + blockIdx.x);                       \
      wt_[slot] = __builtin_amdgcn_s_memrealtime();                                                  \
      if ((slot) == 0)                                                                               \
        wt_[7] = ((long long)__builtin_amdgcn_s_getreg(20 | (31 << 11)) << 32) |                       \
                 (unsigned)__builtin_amdgcn_s_getreg(4 | (31 << 11));                                \
    }                                                                                                \
  } while (0)
#else
#define FSTAMP(id) \
  do {             \
  } while (0)
#define WTRACE(slot) \
  do {               \
  } while (0)
#define WTRACE2(slot) \
  do {                \
  } while (0)
#endif
#ifndef MFGP_SPIN_SLEEP
#define MFGP_SPIN_SLEEP 16
#endif

// (shared device helpers: mfgp_device.h)

// The unit's parts, in dependency order
#include "mfgp_factor.inl"
#include "mfgp_handoff.inl"
#include "mfgp_append.inl"
#include "mfgp_stream.inl"
#include "mfgp_lattice.inl"
#include "mfgp_small.inl"

// ---------------------------------------------------------------------------
#ifdef MFGP_STAMPS
hipError_t set_stamps(long long* p) { return hipMemcpyToSymbol(HIP_SYMBOL(g_stamps), &p, sizeof(p)); }
#endif
hipError_t launch_append(const GPDesc* d, int count, hipStream_t s) {
  hipLaunchKernelGGL(k_append, dim3(count), dim3(64), 0, s, d);
  return hipGetLastError();
}
hipError_t launch_assemble(const GPDesc* d, int count, int64_t max_tiles, hipStream_t s) {
  hipLaunchKernelGGL(k_assemble, dim3((unsigned)max_tiles, count), dim3(NT), 0, s, d);
  return hipGetLastError();
}
hipError_t launch_potrf_diag(const GPDesc* d, int count, int kb, hipStream_t s) {
  hipLaunchKernelGGL(k_potrf_diag, dim3(count), dim3(NT), 0, s, d, kb);
  return hipGetLastError();
}
hipError_t launch_panel(const GPDesc* d, int count, int kb, int64_t max_below, hipStream_t s) {
  hipLaunchKernelGGL(k_panel, dim3((unsigned)max_below, count), dim3(NT), 0, s, d, kb);
  return hipGetLastError();
}
hipError_t launch_syrk(const GPDesc* d, int count, int kb, int64_t max_tri, int t0, hipStream_t s) {
  hipLaunchKernelGGL(k_syrk, dim3((unsigned)max_tri, count), dim3(NT), 0, s, d, kb, t0);
  return hipGetLastError();
}
hipError_t launch_syrk_blk(const GPDesc* d, int count, int kb0, int nk, int jmin, int jmax, int64_t max_tiles,
                           hipStream_t s) {
  if (max_tiles <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_syrk_blk, dim3((unsigned)max_tiles, count), dim3(NT), 0, s, d, kb0, nk, jmin, jmax);
  return hipGetLastError();
}
hipError_t launch_predict(const GPDesc* d, int count, int64_t max_ctiles, hipStream_t s) {
  hipLaunchKernelGGL(k_predict, dim3((unsigned)max_ctiles, count), dim3(PNT), 0, s, d);
  return hipGetLastError();
}
hipError_t launch_extract_z(const GPDesc* d, int count, int64_t max_n, hipStream_t s) {
  if (max_n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_extract_z, dim3((unsigned)((max_n + NT - 1) / NT), count), dim3(NT), 0, s, d);
  return hipGetLastError();
}
hipError_t launch_choi_select_batch(int count, const int* pos, int64_t* state, const int* const* status,
                                    const double* thr, const double* vmax,
                                    const int64_t* vargmax, const double* mu, const int64_t* moff,
                                    const double* const* grids, const int64_t* Ms, double* xn, double* yn,
                                    double* pts, int64_t max_points, hipStream_t s) {
  hipLaunchKernelGGL(k_choi_select_batch, dim3((count + 63) / 64), dim3(64), 0, s, count, pos, state, status, thr, vmax,
                     vargmax, mu, moff, grids, Ms, xn, yn, pts, max_points);
  return hipGetLastError();
}
hipError_t launch_choi_select(const GPDesc* d, double threshold, double* points, int64_t max_points,
                              hipStream_t s) {
  hipLaunchKernelGGL(k_choi_select, dim3(1), dim3(64), 0, s, d, threshold, points, max_points);
  return hipGetLastError();
}
hipError_t launch_inc_stream(const GPDesc* d, int count, int64_t max_blocks, int vf32, hipStream_t s) {
  if (vf32) hipLaunchKernelGGL(k_inc_stream<float>, dim3(count, (unsigned)max_blocks), dim3(NT), 0, s, d);
  else hipLaunchKernelGGL(k_inc_stream<double>, dim3(count, (unsigned)max_blocks), dim3(NT), 0, s, d);
  return hipGetLastError();
}
hipError_t launch_inc_stream_arg(const GPDesc* h, int count, int64_t max_blocks, int vf32, hipStream_t s) {
  if (count < 1 || count > DESC_ARG_MAX) return hipErrorInvalidValue;
  DescArg a;
  std::memcpy(a.d, h, sizeof(GPDesc) * count);
  if (vf32) hipLaunchKernelGGL(k_inc_stream_arg<float>, dim3(count, (unsigned)max_blocks), dim3(NT), 0, s, a);
  else hipLaunchKernelGGL(k_inc_stream_arg<double>, dim3(count, (unsigned)max_blocks), dim3(NT), 0, s, a);
  return hipGetLastError();
}
hipError_t launch_inc_stream1(const GPDesc& d, int64_t blocks, int vf32, hipStream_t s) {
  if (vf32) hipLaunchKernelGGL(k_inc_stream1<float>, dim3(1, (unsigned)blocks), dim3(NT), 0, s, d);
  else hipLaunchKernelGGL(k_inc_stream1<double>, dim3(1, (unsigned)blocks), dim3(NT), 0, s, d);
  return hipGetLastError();
}
hipError_t launch_vstream(const GPDesc* d, int count, int64_t max_ctiles, int vf32, hipStream_t s) {
  if (vf32) hipLaunchKernelGGL(k_vstream<float>, dim3((unsigned)max_ctiles, count), dim3(NT), 0, s, d);
  else hipLaunchKernelGGL(k_vstream<double>, dim3((unsigned)max_ctiles, count), dim3(NT), 0, s, d);
  return hipGetLastError();
}
// The lattice kernels' instance for a launch's (ka, vf32): f(KA, VT()) with KA an
// integral_constant (8 or 16) and VT float or double.
template <class F>
static void by_ka_vt(int ka, int vf32, F f) {
  using K8 = std::integral_constant<int, 8>;
  using K16 = std::integral_constant<int, 16>;
  if (ka == 8 && vf32) f(K8{}, float{});
  else if (ka == 8) f(K8{}, double{});
  else if (vf32) f(K16{}, float{});
  else f(K16{}, double{});
}
hipError_t launch_inc_lat(const GPDesc* d, int count, int64_t max_blocks, int ka, int vf32, bool g1, hipStream_t s) {
  const dim3 g(count, (unsigned)max_blocks);
  by_ka_vt(ka, vf32, [&](auto KA, auto vt) {
    if (g1) hipLaunchKernelGGL((k_inc_lat<KA.value, decltype(vt), true>), g, dim3(NT), 0, s, d);
    else hipLaunchKernelGGL((k_inc_lat<KA.value, decltype(vt), false>), g, dim3(NT), 0, s, d);
  });
  return hipGetLastError();
}
hipError_t launch_inc_lat_arg(const GPDesc* h, int count, int64_t max_blocks, int ka, int vf32, bool g1,
                              hipStream_t s) {
  if (count < 1 || count > DESC_ARG_MAX) return hipErrorInvalidValue;
  DescArg a;
  std::memcpy(a.d, h, sizeof(GPDesc) * count);
  const dim3 g(count, (unsigned)max_blocks);
  by_ka_vt(ka, vf32, [&](auto KA, auto vt) {
    if (g1) hipLaunchKernelGGL((k_inc_lat_arg<KA.value, decltype(vt), true>), g, dim3(NT), 0, s, a);
    else hipLaunchKernelGGL((k_inc_lat_arg<KA.value, decltype(vt), false>), g, dim3(NT), 0, s, a);
  });
  return hipGetLastError();
}
hipError_t launch_lat_gemm2(const GPDesc* d, int count, int64_t max_tiles, int ka, int vf32, hipStream_t s) {
  const dim3 g(count, (unsigned)max_tiles);
  by_ka_vt(ka, vf32, [&](auto KA, auto vt) {
    hipLaunchKernelGGL((k_lat_gemm2<KA.value, decltype(vt)>), g, dim3(G2NT), 0, s, d);
  });
  return hipGetLastError();
}
hipError_t launch_lat_gemm2_arg(const GPDesc* h, int count, int64_t max_tiles, int ka, int vf32, hipStream_t s) {
  if (count < 1 || count > DESC_ARG_MAX) return hipErrorInvalidValue;
  DescArg a;
  std::memcpy(a.d, h, sizeof(GPDesc) * count);
  const dim3 g(count, (unsigned)max_tiles);
  by_ka_vt(ka, vf32, [&](auto KA, auto vt) {
    hipLaunchKernelGGL((k_lat_gemm2_arg<KA.value, decltype(vt)>), g, dim3(G2NT), 0, s, a);
  });
  return hipGetLastError();
}
hipError_t launch_lat_axes(const GPDesc* d, int count, int64_t max_tabw, hipStream_t s) {
  hipLaunchKernelGGL(k_lat_axes, dim3((unsigned)((4 * (max_tabw + 1) + 3) / 4), count), dim3(NT), 0, s, d);
  return hipGetLastError();
}
hipError_t launch_lat_tables(const GPDesc* d, int count, int64_t max_rows, hipStream_t s) {
  if (max_rows <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_lat_tables, dim3((unsigned)((max_rows + 3) / 4), count), dim3(NT), 0, s, d);
  return hipGetLastError();
}
hipError_t launch_vnarrow(const GPDesc* d, int count, int64_t max_tiles, hipStream_t s) {
  if (max_tiles <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_vnarrow, dim3((unsigned)max_tiles, count), dim3(NT), 0, s, d);
  return hipGetLastError();
}

}  // namespace mfgp
