// k_msm_common.hip -- the kernels of the bucket sums and the batch verifications that know no curve, compiled ONCE: the zeroing, the scan and the scatter of
// msm_stages.cuh's schedule (between a unit's digits and its slices) and the AND of the per-lane verdicts.  PUBLIC data only.
// Registers (build/csrc/k_msm_common-hip-amdgcn-amd-amdhsa-gfx950.s; DESIGN.md has the table): 6, 18 and 8 VGPRs for zero, scan and scatter, no scratch.
#include "kernels.h"
#include "msm_stages.cuh"

namespace ecsimd_hip {
namespace {
using launch::BLOCK;

// The words a call counts into -- counter[0] invalid points, counter[1] broken invariants, the histogram behind them; a batch's header block -- zeroed by a
// kernel, as every other node of a captured call is a kernel: 16 bytes per lane.
__global__ void __launch_bounds__(BLOCK) k_msm_zero(uint4* __restrict__ words, size_t n16) {
  const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
  if (i < n16) words[i] = make_uint4(0u, 0u, 0u, 0u);
}

// One workgroup of 1024: lane t sums its `per` consecutive counters, the sums are scanned in LDS, the lane walks its counters again.
__global__ void __launch_bounds__(1024) k_msm_scan(const uint32_t* __restrict__ hist, uint32_t* __restrict__ start, uint32_t* __restrict__ cursor, size_t K) {
  __shared__ uint32_t part[1024];
  const size_t per = (K + 1023) / 1024, t = threadIdx.x;
  const size_t lo = t * per < K ? t * per : K, hi = lo + per < K ? lo + per : K;
  uint32_t sum = 0;
  for (size_t e = lo; e < hi; ++e) sum += hist[e];
  part[t] = sum;
  __syncthreads();
  for (int d = 1; d < 1024; d <<= 1) {
    const uint32_t v = t >= (size_t)d ? part[t - d] : 0u;
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  uint32_t run = part[t] - sum;                                         // exclusive
  for (size_t e = lo; e < hi; ++e) { start[e] = run; cursor[e] = run; run += hist[e]; }
  if (t == 1023) start[K] = part[1023];
}

__global__ void __launch_bounds__(BLOCK) k_msm_scatter(const uint64_t* __restrict__ kk, uint32_t* __restrict__ cursor, uint32_t* __restrict__ sorted, uint32_t* __restrict__ broken, size_t n, size_t T, int c, int windows) {
  const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n) return;
  const uint32_t* kw = reinterpret_cast<const uint32_t*>(kk) + 8 * i;
#pragma unroll 1
  for (int w = 0; w < windows; ++w) {
    const uint32_t pos = atomicAdd(&cursor[((size_t)w << c) + digit_of(kw, w, c)], 1u);
    if (pos < T) sorted[pos] = (uint32_t)i; else atomicAdd(broken, 1u);  // the histogram counted this very digit: anything else fails the call (the units' final kernels)
  }
}

// One workgroup: ok = every one of the n bytes of flags is 1 (and 1 for n = 0).  flags is 16-byte aligned; the bytes behind flags[n - 1] are not read.
__global__ void __launch_bounds__(1024) k_flags_all(const uint8_t* __restrict__ flags, size_t n, uint8_t* __restrict__ okv) {
  const size_t t = threadIdx.x, vec = n / 16;
  const uint4* q = reinterpret_cast<const uint4*>(flags);
  int bad = 0;
  for (size_t v = t; v < vec; v += 1024) {
    const uint4 w = q[v];
    bad |= (int)((w.x != 0x01010101u) | (w.y != 0x01010101u) | (w.z != 0x01010101u) | (w.w != 0x01010101u));
  }
  for (size_t b = vec * 16 + t; b < n; b += 1024) bad |= (int)(flags[b] != 1u);
  const int any = __syncthreads_or(bad);
  if (t == 0) okv[0] = (uint8_t)(any ? 0 : 1);
}
}  // namespace

namespace launch {
void msm_zero(hipStream_t s, void* words, size_t bytes) {
  hipLaunchKernelGGL(k_msm_zero, grid_for(bytes / 16), dim3(BLOCK), 0, s, static_cast<uint4*>(words), bytes / 16);
}
void msm_scan(hipStream_t s, const uint32_t* hist, uint32_t* start, uint32_t* cursor, size_t K) {
  hipLaunchKernelGGL(k_msm_scan, dim3(1), dim3(1024), 0, s, hist, start, cursor, K);
}
void msm_scatter(hipStream_t s, const uint64_t* kk, uint32_t* cursor, uint32_t* sorted, uint32_t* broken, size_t n, size_t T, int c, int windows) {
  hipLaunchKernelGGL(k_msm_scatter, grid_for(n), dim3(BLOCK), 0, s, kk, cursor, sorted, broken, n, T, c, windows);
}
void flags_all(hipStream_t s, const uint8_t* flags, size_t n, uint8_t* ok) {
  hipLaunchKernelGGL(k_flags_all, dim3(1), dim3(1024), 0, s, flags, n, ok);
}
}  // namespace launch
}  // namespace ecsimd_hip
