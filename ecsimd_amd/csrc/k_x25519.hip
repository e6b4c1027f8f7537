// k_x25519.hip -- X25519 (RFC 7748) and the Ed25519 key conversions: the kernels behind ecsimd_x25519 / _base / _from_ed25519_pk / _from_ed25519_seed / _raw.
// x25519.cuh has the ladder, the comb route and the maps; one lane per element; every array is n records of 32 little-endian bytes at any alignment (word
// accesses where its base is a multiple of 4: one flag per array).
//
// SECRET data (selects only; no branch, address or lane mask made of it, nothing declassified, no scratch memory, no LDS -- tools/ct_check.py
// check_secret_flow holds the ISA to that):
//   * k_x25519               out = X25519(scalar, u): clamp, bit 255 of u dropped, the ladder, the canonical x; ok = out is not all zero, by an OR.
//   * k_x25519_base          out = X25519(scalar, 9) through the comb over the multiples of B (M = L's gmod, by value).
//   * k_x25519_from_ed_seed  the clamped low half of SHA-512(seed).
// PUBLIC data:
//   * k_x25519_from_ed_pk    u = (1 + y) / (1 - y) and ok.
//   * k_x25519_raw           one function of the layers below on raw operands (ecsimd_x25519_raw).
#include "kernels.h"
#include "x25519.cuh"

namespace ecsimd_hip {
namespace {
using launch::BLOCK;
#define GID size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x; if (i >= n) return

__global__ void __launch_bounds__(BLOCK) k_x25519(const uint8_t* __restrict__ scalar, uint32_t scalar_aligned, const uint8_t* __restrict__ u, uint32_t u_aligned,
                                                  uint8_t* __restrict__ out, uint32_t out_aligned, uint8_t* __restrict__ ok, size_t n) {
  GID;
  const fe k = x25519_clamp(ed_load32(scalar + 32 * i, scalar_aligned));
  fe x1 = ed_load32(u + 32 * i, u_aligned);
  x1.w[7] &= 0x7fffffffu;
  const fe r = x25519_ladder(k, x1);
  ed_store32(out + 32 * i, r, out_aligned);
  if (ok) ok[i] = (uint8_t)(x25519_nonzero_mask(r) & 1u);
}
__global__ void __launch_bounds__(BLOCK) k_x25519_base(gmod M, const uint8_t* __restrict__ scalar, uint32_t scalar_aligned, uint8_t* __restrict__ out, uint32_t out_aligned,
                                                       size_t n) {
  GID;
  ed_store32(out + 32 * i, x25519_base_ct(x25519_clamp(ed_load32(scalar + 32 * i, scalar_aligned)), M), out_aligned);
}
__global__ void __launch_bounds__(BLOCK) k_x25519_from_ed_pk(const uint8_t* __restrict__ pk, uint32_t pk_aligned, uint8_t* __restrict__ u, uint32_t u_aligned,
                                                             uint8_t* __restrict__ ok, size_t n) {
  GID;
  fe r;
  const uint32_t good = ed_to_mont(r, ed_load32(pk + 32 * i, pk_aligned));
  ed_store32(u + 32 * i, r, u_aligned);
  ok[i] = (uint8_t)(good & 1u);
}
__global__ void __launch_bounds__(BLOCK) k_x25519_from_ed_seed(const uint8_t* __restrict__ seed, uint32_t seed_aligned, uint8_t* __restrict__ scalar, uint32_t scalar_aligned,
                                                               size_t n) {
  GID;
  ed_store32(scalar + 32 * i, x25519_scalar_of_seed(ed_load32(seed + 32 * i, seed_aligned)), scalar_aligned);
}
// records of 32-byte little-endian values, launch::x25519_raw_inputs(op) of them in and x25519_raw_outputs(op) out per lane
__global__ void __launch_bounds__(BLOCK) k_x25519_raw(int op, const uint8_t* __restrict__ in, uint8_t* __restrict__ out, uint32_t aligned, size_t n) {
  GID;
  const int ni = launch::x25519_raw_inputs(op), no = launch::x25519_raw_outputs(op);
  const uint8_t* ip = in + (size_t)32 * ni * i;
  uint8_t* op_ = out + (size_t)32 * no * i;
  const fe a = ed_load32(ip, aligned);
  fe r = fe25519_small(0u), flag = fe25519_small(0u);
  switch (op) {
    case launch::X25519_RAW_FE_MUL_SMALL: r = fe25519_canon(fe25519_mul_small(a, X25519_A24)); break;
    case launch::X25519_RAW_LADDER: r = x25519_ladder(a, ed_load32(ip + 32, aligned)); break;
    case launch::X25519_RAW_ED_TO_MONT: flag = fe25519_small(ed_to_mont(r, a) & 1u); break;
    default: break;
  }
  ed_store32(op_, r, aligned);
  if (no > 1) ed_store32(op_ + 32, flag, aligned);
}
}  // namespace

namespace launch {
static uint32_t word_aligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0 ? 1u : 0u; }
void x25519(hipStream_t s, const uint8_t* scalar, const uint8_t* u, uint8_t* out, uint8_t* ok, size_t n) {
  hipLaunchKernelGGL(k_x25519, grid_for(n), dim3(BLOCK), 0, s, scalar, word_aligned(scalar), u, word_aligned(u), out, word_aligned(out), ok, n);
}
void x25519_base(hipStream_t s, const gmod& L, const uint8_t* scalar, uint8_t* out, size_t n) {
  hipLaunchKernelGGL(k_x25519_base, grid_for(n), dim3(BLOCK), 0, s, L, scalar, word_aligned(scalar), out, word_aligned(out), n);
}
void x25519_from_ed_pk(hipStream_t s, const uint8_t* pk, uint8_t* u, uint8_t* ok, size_t n) {
  hipLaunchKernelGGL(k_x25519_from_ed_pk, grid_for(n), dim3(BLOCK), 0, s, pk, word_aligned(pk), u, word_aligned(u), ok, n);
}
void x25519_from_ed_seed(hipStream_t s, const uint8_t* seed, uint8_t* scalar, size_t n) {
  hipLaunchKernelGGL(k_x25519_from_ed_seed, grid_for(n), dim3(BLOCK), 0, s, seed, word_aligned(seed), scalar, word_aligned(scalar), n);
}
void x25519_raw(hipStream_t s, int op, const uint8_t* in, uint8_t* out, size_t n) {
  hipLaunchKernelGGL(k_x25519_raw, grid_for(n), dim3(BLOCK), 0, s, op, in, out, word_aligned(in) & word_aligned(out), n);
}
}  // namespace launch
}  // namespace ecsimd_hip
