// Full factor and full predict: k_assemble, k_potrf_diag, k_panel, k_syrk, k_syrk_blk,
// k_predict (with its fused variance max / argmax), k_extract_z. Included by mfgp_kernels.hip.

// ---------------------------------------------------------------------------
// Assembly: lower-triangular tiles of the augmented matrix
//   [ K + (sigma_n + jitter) I   .  ]   rows 0..N-1
//   [ (y - m)^T                  1  ]   row N  (its pivot is forced to 1)
//   [ 0                          I  ]   padding up to a multiple of NB
// Grid (tiles, batch); 256 threads; thread -> (row i = tid & 63, column group).
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void k_assemble(const GPDesc* __restrict__ descs) {
  const GPDesc& d = descs[blockIdx.y];
  const int64_t N = d.N, NL = d.NL, ld = d.ld;
  const int64_t T = nblocks_factor(N);
  const int64_t t = blockIdx.x;
  if (t == 0 && threadIdx.x == 0) *d.status = INT_MAX;
  if (t >= T * (T + 1) / 2) return;
  int I, J;
  tri_index(t, I, J);
  const Hyp& h = d.hf;
  const int i = threadIdx.x & 63;
  const int64_t gi = (int64_t)I * NB + i;
  double* __restrict__ A = d.A;
  for (int jj = threadIdx.x >> 6; jj < NB; jj += 4) {
    const int64_t gj = (int64_t)J * NB + jj;
    double v;
    if (gj > gi) {
      v = 0.0;
    } else if (gi < N) {
      v = k_entry(h, d.X, NL, gi, gj);
    } else if (gi == N && gj < N) {
      // residual y - m (gp:133 SF; gp:419-421 MF): lofi rows use mean_L, hifi mean_H
      const double m = (h.kind == 1 && gj < NL) ? h.meanL : h.meanH;
      v = d.y[gj] - m;
    } else {
      v = (gi == gj) ? 1.0 : 0.0;
    }
    A[gj * ld + gi] = v;
  }
}

// ---------------------------------------------------------------------------
// Diagonal block kb: Cholesky of the 64x64 tile and the explicit inverse of its
// factor, blocked in 16x16 sub-blocks so the serial part is four 16-step chains:
//   for each 16-column sub-block: (a) wave 0 factors the 16x16 diagonal block
//   (lane r owns row r in registers, column broadcasts by v_readlane) and inverts
//   it (lane c solves column c); (b) the sub-panel below is multiplied by that
//   inverse; (c) the trailing sub-matrix is updated -- (b) and (c) by all 256
//   threads. Then Linv's off-diagonal 16x16 blocks follow by block substitution.
// Rows >= N (the augmented row and padding) get pivot 1; a non-positive pivot
// on a real row is recorded in *status (LAPACK potrf's INFO, which NumPy turns
// into LinAlgError, gp:254 / gp:529) and replaced by 1 to keep the batch finite.
// ---------------------------------------------------------------------------
// (SP, DB, the DPP broadcasts, mfma16 and factor_invert_64: mfgp_device.h)

__global__ __launch_bounds__(NT) void k_potrf_diag(const GPDesc* __restrict__ descs, int kb) {
  const GPDesc& d = descs[blockIdx.x];
  const int64_t N = d.N, ld = d.ld;
  if (kb >= nblocks_factor(N)) return;
  __shared__ double sh[2 * NB * SP + (NB / DB - 1) * DB * DP];
  double* const S = sh;
  double* const R = sh + NB * SP;
  double* const U = R + NB * SP;
  const int tid = threadIdx.x;
  const int64_t o = (int64_t)kb * NB;
  double* __restrict__ A = d.A;
  STAMP(0);
  {
    // unconditional loads (the upper part of the tile is masked afterwards) keep
    // all 16 loads per thread in flight
    double v[NB * NB / NT];
#pragma unroll
    for (int t = 0; t < NB * NB / NT; ++t) {
      const int e = tid + t * NT, i = e & 63, j = e >> 6;
      v[t] = A[(o + j) * ld + o + i];
    }
#pragma unroll
    for (int t = 0; t < NB * NB / NT; ++t) {
      const int e = tid + t * NT, i = e & 63, j = e >> 6;
      S[i * SP + j] = (j <= i) ? v[t] : 0.0;
    }
  }
  __syncthreads();
  STAMP(1);
  factor_invert_64(S, R, U, o, N, d.status);
  double* __restrict__ Li = d.Linv + (int64_t)kb * TILE;
#pragma unroll 4
  for (int e = tid; e < NB * NB; e += NT) {
    const int i = e & 63, j = e >> 6;   // column-major: consecutive threads -> consecutive rows
    A[(o + j) * ld + o + i] = S[i * SP + j];
    Li[j * NB + i] = R[i * SP + j];
  }
  STAMP(18);
}

// Panel: L_ik = A_ik * Linv_kk^T for every row block i > kb.
__global__ __launch_bounds__(NT) void k_panel(const GPDesc* __restrict__ descs, int kb) {
  const GPDesc& d = descs[blockIdx.y];
  const int64_t nb = nblocks_factor(d.N);
  const int64_t ib = kb + 1 + (int64_t)blockIdx.x;
  if (ib >= nb) return;
  __shared__ double As[TILE], Bs[TILE];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, wm = w >> 1, wn = w & 1;
  load_tile_cm(As, d.A, d.ld, ib * NB, (int64_t)kb * NB, tid);
  load_tile_cm(Bs, d.Linv + (int64_t)kb * TILE, NB, 0, 0, tid);  // Bs[m][j] = Linv[j][m]
  __syncthreads();
  Acc acc;
  acc_zero(acc);
  tile_mma<false>(As, Bs, acc, wm, wn, lane);
  const int r = lane & 15, q = lane >> 4;
  double* __restrict__ A = d.A;
  const int64_t ld = d.ld;
#pragma unroll
  for (int mt = 0; mt < 2; ++mt)
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int row = acc_row(wm, mt, q, v), col = acc_col(wn, nt, r);
        A[((int64_t)kb * NB + col) * ld + ib * NB + row] = acc.c[mt][nt][v];
      }
}

// Trailing update: A_ij -= L_ik L_jk^T for kb < j <= i (lower tiles only).
// Trailing tiles t0, t0+1, ... of step kb (t0 = 1 skips tile (kb+1, kb+1), which
// the look-ahead diagonal kernel updates itself).
__global__ __launch_bounds__(NT) void k_syrk(const GPDesc* __restrict__ descs, int kb, int t0) {
  const GPDesc& d = descs[blockIdx.y];
  const int64_t nb = nblocks_factor(d.N);
  const int64_t T = nb - kb - 1;
  const int64_t t = blockIdx.x + (int64_t)t0;
  if (T <= 0 || t >= T * (T + 1) / 2) return;
  int ii, jj;
  tri_index(t, ii, jj);
  const int64_t ib = kb + 1 + ii, jb = kb + 1 + jj;
  __shared__ double As[TILE], Bs[TILE];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, wm = w >> 1, wn = w & 1;
  const int r = lane & 15, q = lane >> 4;
  const int64_t ld = d.ld;
  double* __restrict__ A = d.A;
  load_tile_cm(As, A, ld, ib * NB, (int64_t)kb * NB, tid);
  load_tile_cm(Bs, A, ld, jb * NB, (int64_t)kb * NB, tid);
  Acc acc;
#pragma unroll
  for (int mt = 0; mt < 2; ++mt)
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int row = acc_row(wm, mt, q, v), col = acc_col(wn, nt, r);
        acc.c[mt][nt][v] = A[(jb * NB + col) * ld + ib * NB + row];
      }
  __syncthreads();
  tile_mma<true>(As, Bs, acc, wm, wn, lane);
#pragma unroll
  for (int mt = 0; mt < 2; ++mt)
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int row = acc_row(wm, mt, q, v), col = acc_col(wn, nt, r);
        A[(jb * NB + col) * ld + ib * NB + row] = acc.c[mt][nt][v];
      }
}

// Trailing update over nk consecutive 64-column steps kb0 .. kb0 + nk - 1 at once
// (two-level blocking): A_ij -= sum_k L_ik L_jk^T for the lower tiles with jmin <=
// j <= min(i, jmax). The accumulator stays in registers across the nk steps and
// the MFMA sequence is k_syrk's, step after step, so the result is bit-equal to nk
// k_syrk launches; the tile is read and written once instead of nk times, and
// the next step's two operand tiles load while this step's MFMAs run.
__global__ __launch_bounds__(NT) void k_syrk_blk(const GPDesc* __restrict__ descs, int kb0, int nk, int jmin,
                                                 int jmax) {
  const GPDesc& d = descs[blockIdx.y];
  const int64_t nb = nblocks_factor(d.N);
  if (kb0 >= nb) return;
  const int64_t jm = jmax < nb - 1 ? jmax : nb - 1;
  if (jmin > jm) return;
  // tile t: column j (from jmin), row i >= j
  int64_t t = blockIdx.x, ib = -1, jb = -1;
  if (jm == nb - 1) {   // a triangle
    const int64_t T = nb - jmin;
    if (t >= T * (T + 1) / 2) return;
    int ii, jj;
    tri_index(t, ii, jj);
    ib = jmin + ii;
    jb = jmin + jj;
  } else {              // a few columns
    for (int64_t j = jmin; j <= jm; ++j) {
      if (t < nb - j) {
        ib = j + t;
        jb = j;
        break;
      }
      t -= nb - j;
    }
    if (ib < 0) return;
  }
  const int kn = (int)(kb0 + nk <= nb ? nk : nb - kb0);
  __shared__ double As[TILE], Bs[TILE];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, wm = w >> 1, wn = w & 1;
  const int r = lane & 15, q = lane >> 4;
  const int64_t ld = d.ld;
  double* __restrict__ A = d.A;
  TileRegs ra, rb;
  tile_fetch(ra, A + (int64_t)kb0 * NB * ld + ib * NB, ld, tid);
  tile_fetch(rb, A + (int64_t)kb0 * NB * ld + jb * NB, ld, tid);
  Acc acc;
#pragma unroll
  for (int mt = 0; mt < 2; ++mt)
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int row = acc_row(wm, mt, q, v), col = acc_col(wn, nt, r);
        acc.c[mt][nt][v] = A[(jb * NB + col) * ld + ib * NB + row];
      }
  for (int s = 0; s < kn; ++s) {
    if (s > 0) __syncthreads();   // the previous step's LDS reads are done
    tile_put_k(As, ra, tid);
    tile_put_k(Bs, rb, tid);
    __syncthreads();
    if (s + 1 < kn) {
      const int64_t kc = (int64_t)(kb0 + s + 1) * NB;
      tile_fetch(ra, A + kc * ld + ib * NB, ld, tid);
      tile_fetch(rb, A + kc * ld + jb * NB, ld, tid);
    }
    tile_mma<true>(As, Bs, acc, wm, wn, lane);
  }
#pragma unroll
  for (int mt = 0; mt < 2; ++mt)
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int row = acc_row(wm, mt, q, v), col = acc_col(wn, nt, r);
        A[(jb * NB + col) * ld + ib * NB + row] = acc.c[mt][nt][v];
      }
}

// ---------------------------------------------------------------------------
// Fused predict. One workgroup (256 threads, 4 waves; two workgroups per CU) =
// one GP x 64 grid cells. For each 128-row block I of the training set
// (sequential, left-looking):
//   acc  = psi_I^T                          (exp in registers, gp:139 / gp:426-429)
//   acc -= sum_{J<I} L_IJ V_J               (f64 MFMA over 16-deep K steps)
//   V_I  = L_II^-1 acc                      (two 64-row halves, 64-wide inverses:
//          V_top = Linv_a acc_top;  V_bot = Linv_b (acc_bot - L_ba V_top))
//   var_part += colsum(V_I o V_I);  mu_part += V_I^T z_I
// then mu = m + mu_part (gp:142-143 / gp:432), var = k** - var_part (diag of
// gp:146 / gp:435-436). z = L^-1 (y - m) is read from zv (row N of the
// augmented factor, extracted by k_extract_z). Every V block is stored: V stays
// resident in HBM for the incremental predicts (k_vstream) that follow appends.
//
// Staging: global_load_lds_dwordx4 (LDS-DMA) into a 3-stage ring of 16-deep K
// steps (16 KB of L + 8 KB of V per stage) with two steps in flight, a counted
// vmcnt and one raw s_barrier per step (no __syncthreads in the loop: its fence
// would drain the DMA). The XOR swizzles of the LDS images are applied on the
// global source addresses (the DMA writes lane-linear). All LDS lives in one
// array (hipcc vmcnt trap). The V panels of earlier row blocks are re-read from
// HBM N/256 times -- the 128-row blocks halve that traffic against 64-row ones;
// the second workgroup on the CU hides each one's psi / diagonal phases.
// ---------------------------------------------------------------------------
// (the ring constants, the LDS-DMA forms, main_mma, load_afrag and half_mma: mfgp_device.h)

// Fused np.amax / np.argmax of a GP's variance (simulator.py:672, 842, 1014 and
// the argmax of compute_sample_points, sim:352). Every cell tile publishes its
// (max, first argmax) from its epilogue; the last tile to arrive reduces them.
// The hand-off avoids device-scope fences (a release fence per workgroup would
// write back the XCD's L2 each time): the partial is stored with an agent-scope
// atomic store (write-through), drained with s_waitcnt, then the arrival counter
// is bumped; the last arriver reads the partials with agent-scope atomic loads
// and resets the counter for the next launch. Called by wave 0 of the tile's
// workgroup, lane l holding cell c0 + l (valid if inside the grid).

__device__ void var_argmax_tile(const GPDesc& d, double v, int64_t c, bool valid, int64_t tile) {
  const int lane = threadIdx.x & 63;
  double bv = valid ? v : -__builtin_inf();
  int64_t bi = valid ? c : INT64_MAX;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) argmax_pair(bv, bi, __shfl_xor(bv, off), __shfl_xor(bi, off));
  const int64_t ntiles = ntiles_grid(d.M);
  unsigned* cnt = reinterpret_cast<unsigned*>(d.tred);   // tred = [counter | (max, argmax) per tile]
  double* part = d.tred + 1;
  unsigned old = 0;
  if (lane == 0) {
    __hip_atomic_store(part + 2 * tile, bv, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(part + 2 * tile + 1, (double)bi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    old = __hip_atomic_fetch_add(cnt, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  old = __shfl(old, 0);
  if (old != (unsigned)(ntiles - 1)) return;
  bv = -__builtin_inf();
  bi = INT64_MAX;
  for (int64_t t = lane; t < ntiles; t += 64)
    argmax_pair(bv, bi, __hip_atomic_load(part + 2 * t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT),
                (int64_t)__hip_atomic_load(part + 2 * t + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) argmax_pair(bv, bi, __shfl_xor(bv, off), __shfl_xor(bi, off));
  if (lane == 0) {
    if (d.vmax) *d.vmax = bv;
    if (d.vargmax) *d.vargmax = bi;
    __hip_atomic_store(cnt, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

__global__ __launch_bounds__(PNT, 2) void k_predict(const GPDesc* __restrict__ descs) {
  const GPDesc& d = descs[blockIdx.y];
  const int64_t M = d.M;
  const int64_t c0 = (int64_t)blockIdx.x * PBM;
  if (c0 >= M) return;
  // ring: stage s at lds[s*STAGE] = As [KS][128] then Bs [KS][64]; the diagonal
  // step reuses the ring as the [128][64] image of acc / V (64 KB <= 72 KB).
  __shared__ double lds[NSTAGE * STAGE + PRB];
  double* const zs = lds + NSTAGE * STAGE;
  double* const img = lds;
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave id (uniform)
  const int r = lane & 15, q = lane >> 4;
  const int p16 = w * 16;   // diagonal-step rows of this wave inside a 64-row half
  const Hyp& h = d.hp;
  const int64_t N = d.N, NL = d.NL, ld = d.ld;
  const int64_t nrb = prow_blocks(N);
  const int64_t nbf = nblocks_factor(N);
  const double* __restrict__ X = d.X;
  const double* __restrict__ Amat = d.A;
  double* __restrict__ Vt = d.V + (int64_t)blockIdx.x * d.vld * PBM;   // resident V tile
  double vsum[4] = {0.0, 0.0, 0.0, 0.0}, msum[4] = {0.0, 0.0, 0.0, 0.0};
  // DMA plan of one K step (kc = first factor column / V row of the step):
  //  L image [KS][128]: wave w moves rows k = w + 4j (j < 4), all of parity w&1;
  //    src = A[(kc + k)*ld + base + ((2*lane) ^ sw)]
  //  V image [KS][64]:  wave w moves row pairs p = w + 4j (j < 2), rows 2p + (lane>>5);
  //    src = Vt[(kc + 2p + (lane>>5))*64 + (((lane&31)*2) ^ ((lane>>5)<<4))]
  const __amdgpu_buffer_rsrc_t rsA = make_rsrc(Amat, (int64_t)8 * ld * ld);
  const __amdgpu_buffer_rsrc_t rsV = make_rsrc(Vt, (int64_t)8 * d.vld * PBM);
  const unsigned voffA = (unsigned)(8 * ((2 * lane) ^ ((w & 1) << 4)));
  const unsigned voffV =
      (unsigned)(8 * ((lane >> 5) * PBM + (((lane & 31) * 2) ^ ((lane >> 5) << 4))));
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
    const int nk = (int)(base / KS);   // K steps: all columns left of the block
    // prologue: steps 0 and 1 in flight while psi is generated
#pragma unroll
    for (int s0 = 0; s0 < 2; ++s0) {
      if (s0 < nk) dma_step(lds + s0 * STAGE, base, (int64_t)s0 * KS);
    }
    AccP acc;
    {
      // this lane's four grid cells (columns nt*16 + r), scaled by the length scales
      double cLx[4], cLy[4], cHx[4], cHy[4];
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) {
        int64_t c = c0 + nt * 16 + r;
        if (c >= M) c = M - 1;
        const double gx = d.grid[2 * c], gy = d.grid[2 * c + 1];
        cLx[nt] = div_(gx, h.lL);
        cLy[nt] = div_(gy, h.lL);
        cHx[nt] = div_(gx, h.lH);
        cHy[nt] = div_(gy, h.lH);
      }
#pragma unroll
      for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          const int64_t g = base + w * 32 + mt * 16 + q + 4 * v;
          double pv[4] = {0.0, 0.0, 0.0, 0.0};
          if (g < N) {
            const double tx = X[2 * g], ty = X[2 * g + 1];
            const double tLx = div_(tx, h.lL), tLy = div_(ty, h.lL);
            if (h.kind == 0) {
#pragma unroll
              for (int nt = 0; nt < 4; ++nt) pv[nt] = se_scaled(cLx[nt], cLy[nt], tLx, tLy, h.sL);
            } else if (g < NL) {
#pragma unroll
              for (int nt = 0; nt < 4; ++nt) pv[nt] = h.rho * se_scaled(cLx[nt], cLy[nt], tLx, tLy, h.sL);
            } else {
              const double tHx = div_(tx, h.lH), tHy = div_(ty, h.lH);
#pragma unroll
              for (int nt = 0; nt < 4; ++nt) {
#pragma clang fp contract(off)
                pv[nt] = h.rho2 * se_scaled(cLx[nt], cLy[nt], tLx, tLy, h.sL) +
                         se_scaled(cHx[nt], cHy[nt], tHx, tHy, h.sH);
              }
            }
          }
#pragma unroll
          for (int nt = 0; nt < 4; ++nt) acc.c[mt][nt][v] = -pv[nt];   // acc = -psi + sum L V
        }
    }
    double frag[16];
    if (nk > 0) {
      // step 0 landed (step 1 may still be in flight)
      if (nk > 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(GLDS_PER_STEP) : "memory");
      else vm_wait_all();
      __builtin_amdgcn_s_barrier();
    }
    // acc += L_I,<I V_<I over 16-deep steps; steps s+1, s+2 in flight during step s
    for (int s = 0; s < nk; ++s) {
      const double* cur = lds + (s % NSTAGE) * STAGE;
      if (s + 2 < nk) dma_step(lds + ((s + 2) % NSTAGE) * STAGE, base, (int64_t)(s + 2) * KS);
      main_mma(cur, cur + KS * PW, acc, w, lane);
      if (s + 2 < nk) asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"(GLDS_PER_STEP) : "memory");
      else asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");
    }
    // ---- diagonal block: V_I = L_II^-1 (psi - L V), two 64-row halves ----
    const int64_t fa = 2 * I, fb = 2 * I + 1;       // 64-blocks of the factor
    const bool has_b = fb < nbf;                    // bottom half holds real rows
    load_afrag(frag, d.Linv + fa * TILE, NB, p16, lane);   // Linv_a
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int nt = 0; nt < 4; ++nt)
#pragma unroll
        for (int v = 0; v < 4; ++v) img[swz(w * 32 + mt * 16 + q + 4 * v, nt * 16 + r)] = -acc.c[mt][nt][v];
    if (tid < PRB) {
      const int64_t g = base + tid;
      zs[tid] = (g < N) ? d.zv[g] : 0.0;
    }
    __syncthreads();
    // V_top = Linv_a * T_top (Linv_a lower triangular: rows p16.. need K < p16 + 16)
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
        const double val = vh.c[nt][v];
        gp(Vt)[(base + row) * PBM + col] = val;
        if (base + row < N) {
          vsum[nt] += val * val;
          msum[nt] += val * zs[row];
        }
      }
    __syncthreads();   // every wave is done reading T_top
    if (has_b) {
#pragma unroll
      for (int nt = 0; nt < 4; ++nt)
#pragma unroll
        for (int v = 0; v < 4; ++v) img[swz(p16 + q + 4 * v, nt * 16 + r)] = vh.c[nt][v];
      __syncthreads();
      // T_bot -= L_ba V_top   (each wave: its own 16 rows of the bottom half)
      AccH th;
#pragma unroll
      for (int nt = 0; nt < 4; ++nt)
#pragma unroll
        for (int v = 0; v < 4; ++v) th.c[nt][v] = img[swz(64 + p16 + q + 4 * v, nt * 16 + r)];
      half_mma<true>(frag, img, 0, th, 16, lane);
      load_afrag(frag, d.Linv + fb * TILE, NB, p16, lane);   // Linv_b
#pragma unroll
      for (int nt = 0; nt < 4; ++nt)
#pragma unroll
        for (int v = 0; v < 4; ++v) img[swz(64 + p16 + q + 4 * v, nt * 16 + r)] = th.c[nt][v];
      __syncthreads();
      // V_bot = Linv_b T_bot
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) vh.c[nt] = d4{0.0, 0.0, 0.0, 0.0};
      half_mma<false>(frag, img, 64, vh, (p16 + 16) / 4, lane);
#pragma unroll
      for (int nt = 0; nt < 4; ++nt)
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          const int row = 64 + p16 + q + 4 * v, col = nt * 16 + r;
          const double val = vh.c[nt][v];
          gp(Vt)[(base + row) * PBM + col] = val;
          if (base + row < N) {
            vsum[nt] += val * val;
            msum[nt] += val * zs[row];
          }
        }
    }
    vm_wait_all();      // V_I stores complete before any later DMA reads them
    __syncthreads();    // and before the next prologue overwrites the LDS images
  }
  // reduce over the 4 row groups of the wave (lanes r, r+16, r+32, r+48), then
  // over the 4 waves (LDS, reusing the ring)
#pragma unroll
  for (int nt = 0; nt < 4; ++nt) {
    vsum[nt] += __shfl_xor(vsum[nt], 16);
    vsum[nt] += __shfl_xor(vsum[nt], 32);
    msum[nt] += __shfl_xor(msum[nt], 16);
    msum[nt] += __shfl_xor(msum[nt], 32);
  }
  double* red = lds;   // [2][4][PBM]
  if (q == 0) {
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
      red[(0 * 4 + w) * PBM + nt * 16 + r] = vsum[nt];
      red[(1 * 4 + w) * PBM + nt * 16 + r] = msum[nt];
    }
  }
  __syncthreads();
  if (tid < PBM) {
    const int64_t c = c0 + tid;
    const double vs = (red[0 * PBM + tid] + red[1 * PBM + tid]) + (red[2 * PBM + tid] + red[3 * PBM + tid]);
    const double ms = (red[4 * PBM + tid] + red[5 * PBM + tid]) + (red[6 * PBM + tid] + red[7 * PBM + tid]);
    const double vc = h.kss - vs;
    if (c < M) {
      d.mu[c] = ms + h.meanH;
      d.var[c] = vc;
      if (d.rmu) {
        d.rmu[c] = ms + h.meanH;
        d.rvar[c] = vc;
      }
    }
    if (d.vmax || d.vargmax) var_argmax_tile(d, vc, c, c < M, blockIdx.x);
  }
}

// z = L^-1 (y - m) out of row N of the augmented factor into zv (after the
// full factor; the incremental kernels extend zv themselves).
__global__ __launch_bounds__(NT) void k_extract_z(const GPDesc* __restrict__ descs) {
  const GPDesc& d = descs[blockIdx.y];
  const int64_t j = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (j < d.N) d.zv[j] = d.A[j * d.ld + d.N];
}
