// Hand-off primitives of the launches whose workgroups pass data to each other
// (k_inc_stream, k_inc_lat): write-through stores, drains, flags and the bounded
// waits. Included by mfgp_kernels.hip.
//
// Why the in-kernel hand-off is safe (gfx950: 8 XCDs, each with its own L2;
// per-CU L1; kernel boundaries write back and invalidate both):
//  * Forward progress. The dispatcher hands workgroups to the XCDs round-robin
//    in linear order (x = GP fastest, then role) and each XCD dispatches its
//    share in that order. Every producer has a lower linear id than every cell
//    workgroup, so on each XCD all its producers are dispatched before any of its
//    cell workgroups, and producers wait for nothing (the last arriver's finish
//    included). Producers therefore always run to completion even when they do
//    not all fit at once (configs[4]: 32 GPs x 64 producers = 2048 > 1024 slots),
//    and the cells waiting for them are released. The waits are bounded anyway
//    (~1 s, then MFGP_ERR_DEVICE via *status), and tests/test_codeobj.py checks
//    the code has no out-of-line calls (an outlined producer stalled it once).
//  * Visibility. Everything a producer hands over (L21 rows in A, the compact
//    rows, chunk partials, L22 record, z2) is stored with agent-scope atomic
//    stores (global_store ... sc1: written through the XCD's L2 to memory), then
//    drained (s_waitcnt vmcnt(0): the stores are acknowledged), and only then is
//    the flag stored (sc1). A consumer reads the flag with an agent-scope load
//    (sc1: not served from a stale L2 line). Data behind the flag is then read
//    either with sc1 loads (ldx<true>) or with plain loads of lines that no
//    workgroup of the launch reads before the flag is up (compact rows only after
//    every chunk's flag, the L22 record only after sync[2]); such a line cannot
//    be in this XCD's L2 or this CU's L1 (both invalidated at the kernel
//    boundary, never filled since), so the plain load fetches the written data.
//  * Cost. A release (buffer_wbl2 sc1) writes back the whole L2 -- +80 us per
//    step when 2048 workgroups did it -- and an acquire adds a buffer_inv sc1;
//    the construction above needs neither, at the price of the two rules: drain
//    before the flag, and no early read of a handed-over line.

// Data handed between workgroups of ONE launch (k_inc_stream) goes through
// write-through stores and L2-bypassing loads (relaxed, agent scope); each
// producer drains its stores (s_waitcnt) before it signals. No fence: a
// __threadfence writes the whole L2 back. XW = false: plain accesses (the
// consumers are later launches).
template <bool XW>
__device__ __forceinline__ double ldx(const double* p) {
  if constexpr (XW) return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  else return *p;
}
template <bool XW>
__device__ __forceinline__ void stx(double* p, double v) {
  if constexpr (XW) __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  else *p = v;
}
__device__ __forceinline__ void drain_stores() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
// A workgroup barrier that orders LDS only: this wave's LDS accesses complete, then
// s_barrier. Loads in flight stay in flight (__syncthreads' workgroup fence waits for
// them); for LDS data exchanged between the waves of one workgroup.
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }
// 16-byte write-through store (global_store_dwordx4 ... sc1): a whole line per wave
// instruction where 8 lanes cover it, and no dirty line left in the XCD's L2 for the
// launch's end to write back (MI355X_MICROARCH.md: 16-B sc1 stores cost as plain ones)
__device__ __forceinline__ void st16_wt(double* p, dv2 v) {
  asm volatile("global_store_dwordx4 %0, %1, off sc1" ::"v"(p), "v"(v) : "memory");
}
// The consumer's side of a hand-off. Every byte handed between workgroups of one
// launch is stored write-through (sc1, drained before the flag) and loaded with
// device-scope (sc1) loads that L2 does not serve from a possibly stale line, or
// read plain only when no workgroup of that XCD can have cached the line earlier
// in the launch (L2 is invalidated at kernel start); the consumer issues its
// loads after it saw the flag (no speculation). No acquire: an agent-scope
// acquire after each wait (its L2 invalidate) cost the lattice step 105 -> 172 us
// per launch at B = 8, and even one per wait on the polling lane 8 % (97.0k vs
// 89.2k GP-updates/s, round 5): DESIGN 2.2. tests/test_codeobj.py checks the
// emitted polls (sc1 loads, completed before the branch that leaves the spin).
__device__ __forceinline__ void publish(unsigned* f, unsigned v) {
  __hip_atomic_store(f, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// One poll of a hand-off word: a device-scope (sc1) load.
__device__ __forceinline__ bool flag_is(const unsigned* f, unsigned v) {
  return __hip_atomic_load(f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == v;
}
// The bounded spin every wait below is: poll (`done`, what this lane reads), sleep, and
// after ~1 s (1 << 22 polls) record a synchronisation failure in *status (`writer`: the lane
// that writes it; reported by the host) and go on, so a lost signal can never hang the device.
constexpr int SYNC_FAIL = INT_MIN;
template <class Done>
__device__ __forceinline__ void spin_until(const GPDesc& d, bool writer, Done done) {
  int it = 0;
  while (!done()) {
    __builtin_amdgcn_s_sleep(MFGP_SPIN_SLEEP);
    if (++it == (1 << 22)) {
      if (writer) atomicMin(d.status, SYNC_FAIL);
      break;
    }
  }
}
// Wait (thread 0, the workgroup joins at the barrier) until *f == v.
__device__ void wait_flag(const GPDesc& d, const unsigned* f, unsigned v) {
  if (threadIdx.x == 0) spin_until(d, true, [&] { return flag_is(f, v); });
  __syncthreads();
}
// Spin (this wave) until *f == v.
__device__ __forceinline__ void spin_wave(const GPDesc& d, const unsigned* f, unsigned v) {
  spin_until(d, (threadIdx.x & 63) == 0, [&] { return flag_is(f, v); });
}
// Wait (wave 0 polls, the workgroup joins at the barrier) until flags f[0, n) all hold the epoch.
__device__ void wait_flags_all(const GPDesc& d, const unsigned* f, int64_t n, unsigned epoch) {
  if (threadIdx.x < 64) {
    const int lane = threadIdx.x;
    spin_until(d, lane == 0, [&] {
      bool mine = true;
      for (int64_t i = lane; i < n; i += 64) mine = mine && flag_is(f + i, epoch);
      return __ballot(!mine) == 0;
    });
  }
  __syncthreads();
}
// Wait (wave 0 polls; the workgroup joins at the barrier) until rows [lo, n0) of this
// append's compact rows are stored: every producer chunk from lo / FUSED_CHUNK on holds this
// launch's epoch, or sync[1] does (raised by the last producer to arrive, or by the finish
// when it solved L21 itself).
__device__ void wait_l21_from(const GPDesc& d, int64_t lo) {
  if (threadIdx.x < 64) {
    const int lane = threadIdx.x;
    spin_until(d, lane == 0, [&] {
      bool mine = true;
      for (int64_t c = lo / FUSED_CHUNK + lane; c < d.nprod; c += 64) mine = mine && flag_is(d.pflag + c, d.epoch);
      const bool any = flag_is(d.sync + 1, d.epoch);
      return any || __ballot(!mine) == 0;
    });
  }
  __syncthreads();
}
