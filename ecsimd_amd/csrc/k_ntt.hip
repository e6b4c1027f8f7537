// k_ntt.hip -- the number-theoretic transform over any registered prime field (include/ecsimd_ntt.h): one pass of the Stockham split per launch, a tile of
// 2^11 elements per workgroup in LDS, and the bit-reversal permutation.  ntt.cuh has the schedule, the index arithmetic and the pass body, shared with the host;
// this unit supplies the field -- gfield.cuh's g_add / g_sub / g_mul on the by-value gmod (wave-uniform, in SGPRs) -- and the launches.
//
// PUBLIC OR SECRET-INDEPENDENT: every address and every branch is a function of (log_n, batch, flags) and the lane's index; the values only pass through
// gfield.cuh's selects.
#include "kernels.h"
#include "gfield.cuh"
#include "ntt.cuh"

namespace ecsimd_hip {
namespace {

// ntt.cuh's field over gfield.cuh: an element moves as two dwordx4 / two ds_*_b128
struct dev_field {
  typedef fe el;
  const gmod& M;
  ECS_DEV static fe load(const ntt::u4& a, const ntt::u4& b) {
    fe r;
#pragma unroll
    for (int i = 0; i < 4; ++i) { r.w[i] = a.v[i]; r.w[4 + i] = b.v[i]; }
    return r;
  }
  ECS_DEV static void store(const fe& v, ntt::u4* a, ntt::u4* b) {
    ntt::u4 x, y;
#pragma unroll
    for (int i = 0; i < 4; ++i) { x.v[i] = v.w[i]; y.v[i] = v.w[4 + i]; }
    *a = x; *b = y;
  }
  ECS_DEV fe add(const fe& a, const fe& b) const { return g_add(a, b, M); }
  ECS_DEV fe sub(const fe& a, const fe& b) const { return g_sub(a, b, M); }
  ECS_DEV fe mul(const fe& a, const fe& b) const { return g_mul(a, b, M); }
  ECS_DEV fe rsq() const { return g_words(M.rsq); }
  ECS_DEV static fe one() {
    fe r;
#pragma unroll
    for (int i = 0; i < 8; ++i) r.w[i] = i == 0 ? 1u : 0u;
    return r;
  }
};

__global__ void __launch_bounds__(ntt::LANES) k_ntt_pass(gmod M, ntt::pass_args A) {
  __shared__ ntt::u4 lds[ntt::LDS_SLOTS];
  const dev_field F{M};
  const uint64_t tile = blockIdx.x;
  const int lane = (int)threadIdx.x;
  ntt::pass_load(F, A, tile, lane, lds);
  __syncthreads();
#pragma unroll 1
  for (int u = 0; u < A.G.log_r; ++u) {
    ntt::pass_stage(F, A, tile, lane, u, lds);
    __syncthreads();
  }
  ntt::pass_store(F, A, tile, lane, lds);
}

// out[rev(i)] = in[i] in each of `batch` arrays of 2^log_n elements: the lane of i <= rev(i) moves both elements of the pair, so out may be in
__global__ void __launch_bounds__(launch::BLOCK) k_ntt_bitrev(const uint4* in, uint4* out, int log_n, size_t total) {
  const size_t e = (size_t)blockIdx.x * launch::BLOCK + threadIdx.x;
  if (e >= total) return;
  const uint32_t i = (uint32_t)(e & (((size_t)1 << log_n) - 1)), r = ntt::bitrev(i, log_n);
  if (i > r) return;
  const size_t base = e - i, a = base + i, b = base + r;
  const uint4 a0 = in[2 * a], a1 = in[2 * a + 1], b0 = in[2 * b], b1 = in[2 * b + 1];
  out[2 * b] = a0; out[2 * b + 1] = a1;
  out[2 * a] = b0; out[2 * a + 1] = b1;
}
}  // namespace

namespace launch {
void ntt_pass(hipStream_t s, const gmod& M, const ntt::pass_args& A) {
  hipLaunchKernelGGL(k_ntt_pass, dim3((unsigned)ntt::tiles_of(A.G)), dim3(ntt::LANES), 0, s, M, A);
}
void ntt_bitrev(hipStream_t s, const uint64_t* in, uint64_t* out, int log_n, size_t batch) {
  const size_t total = batch << log_n;
  hipLaunchKernelGGL(k_ntt_bitrev, grid_for(total), dim3(BLOCK), 0, s, reinterpret_cast<const uint4*>(in), reinterpret_cast<uint4*>(out), log_n, total);
}
}  // namespace launch
}  // namespace ecsimd_hip
