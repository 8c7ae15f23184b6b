// The small kernels: k_vnarrow, k_choi_select, k_choi_select_batch, k_append.
// Included by mfgp_kernels.hip.

// MFGP_F32 full predict: k_predict computed V in fp64 into the scratch d.V (the
// left-looking solve re-reads its own earlier rows, so it runs in fp64); rows
// [0, N) of every tile are rounded into the resident fp32 V. One workgroup per
// tile, 16-byte loads / 8-byte stores along the rows.
__global__ __launch_bounds__(NT) void k_vnarrow(const GPDesc* __restrict__ descs) {
  const GPDesc& d = descs[blockIdx.y];
  const int64_t t = blockIdx.x;
  if (t >= ntiles_grid(d.M)) return;
  const GLOBAL dv2* src = reinterpret_cast<const GLOBAL dv2*>(gp(d.V) + t * d.vld * PBM);
  GLOBAL float* dst = gp(d.Vf) + t * d.vld * PBM;
  const int64_t n2 = d.N * (PBM / 2);
  for (int64_t e = threadIdx.x; e < n2; e += NT) {
    const dv2 v = __builtin_nontemporal_load(src + e);
    typedef float fv2 __attribute__((ext_vector_type(2)));
    *reinterpret_cast<GLOBAL fv2*>(dst + 2 * e) = fv2{(float)v.x, (float)v.y};
  }
}

// One iteration of compute_sample_points (simulator.py:344-370) on the device:
// the cell of maximal posterior variance (its first occurrence, np.argmax) is
// appended as hifi row N - 1 with its posterior mean as the observation
// (sim:352-366), unless the maximal variance is at or below the threshold or
// max_points rows were chosen -- then the loop is over: *gate = 0 and every
// gated kernel after it is a no-op. state[1] counts the chosen points.
// The model's status word still holds the previous iteration's verdict here: a
// failed append (not positive definite, or a hand-off that never arrived) closes
// the gate too, so no later launch of the chunk resets the word and the host's
// one read at the chunk's end sees the failure.
__global__ void k_choi_select(const GPDesc* __restrict__ descs, double threshold, double* __restrict__ points,
                              int64_t max_points) {
  const GPDesc& d = descs[0];
  if (threadIdx.x != 0 || *d.gate == 0) return;
  int64_t* cnt = reinterpret_cast<int64_t*>(d.gate) + 1;
  const double vmax = *d.vmax;
  const int64_t j = *d.vargmax;
  if (*d.status != INT_MAX || !(vmax > threshold) || *cnt >= max_points || j < 0 || j >= d.M) {
    *d.gate = 0;
    return;
  }
  const int64_t row = d.N - 1;
  const double gx = d.grid[2 * j], gy = d.grid[2 * j + 1];
  const_cast<double*>(d.X)[2 * row] = gx;
  const_cast<double*>(d.X)[2 * row + 1] = gy;
  const_cast<double*>(d.y)[row] = d.mu[j];
  points[2 * *cnt] = gx;
  points[2 * *cnt + 1] = gy;
  *cnt += 1;
}

// The batched form (mfgp_batch_sample_points): thread b decides for model b of the
// batch from its fused (max, argmax) -- stop at its threshold or its point budget
// (state[b] = {gate, count}), else take the argmax cell and its posterior mean as the
// next hifi row, staged in xn / yn at the model's place pos[b] among the batch
// step's members (its device-source rows), and record it in pts[b][count]. A model
// whose previous append failed (status[b], as in k_choi_select) stops as well.
__global__ void k_choi_select_batch(int count, const int* __restrict__ pos, int64_t* __restrict__ state,
                                    const int* const* __restrict__ status, const double* __restrict__ thr,
                                    const double* __restrict__ vmax, const int64_t* __restrict__ vargmax,
                                    const double* __restrict__ mu, const int64_t* __restrict__ moff,
                                    const double* const* __restrict__ grids, const int64_t* __restrict__ Ms,
                                    double* __restrict__ xn, double* __restrict__ yn, double* __restrict__ pts,
                                    int64_t max_points) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= count) return;
  int64_t* st = state + 2 * b;
  if (st[0] == 0) return;
  const double v = vmax[b];
  const int64_t j = vargmax[b], cnt = st[1];
  if (*status[b] != INT_MAX || !(v > thr[b]) || cnt >= max_points || j < 0 || j >= Ms[b]) {
    st[0] = 0;
    return;
  }
  const double gx = grids[b][2 * j], gy = grids[b][2 * j + 1];
  const int p = pos[b];
  xn[2 * p] = gx;
  xn[2 * p + 1] = gy;
  yn[p] = mu[moff[b] + j];
  pts[2 * (b * max_points + cnt)] = gx;
  pts[2 * (b * max_points + cnt) + 1] = gy;
  st[1] = cnt + 1;
}

// Append the batch's new (device-resident) rows to every model's training set:
// one launch for the whole batch instead of two copies per model (full-refactor
// path; k_inc_l21 lands the rows of the bordered appends itself).
__global__ __launch_bounds__(64) void k_append(const GPDesc* __restrict__ descs) {
  const GPDesc& d = descs[blockIdx.x];
  const int64_t kn = d.k_new;
  if (kn <= 0 || !d.srcX) return;
  double* X = const_cast<double*>(d.X);
  double* y = const_cast<double*>(d.y);
  const int64_t at = d.N - kn;
  for (int64_t e = threadIdx.x; e < 3 * kn; e += 64) {
    if (e < 2 * kn) X[2 * at + e] = d.srcX[e];
    else y[at + e - 2 * kn] = d.srcY[e - 2 * kn];
  }
}
