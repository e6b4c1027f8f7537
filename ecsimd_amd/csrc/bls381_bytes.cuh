// bls381_bytes.cuh -- what k_bls12_381.hip (G1) and k_bls12_381_g2.hip (G2) share below the group: 48-byte big-endian records at any alignment, and fe381
// elements in the workspace (48 bytes, three uint4, element e of an array at byte 48 e).  Device only.
#pragma once
#include "kernels.h"
#include "fe381.cuh"
#include "field.cuh"

namespace ecsimd_hip {
// ---- bytes
ECS_DEV fe381 be48_load(const uint8_t* __restrict__ p, uint32_t aligned) {
  fe381 r;
  if (aligned) {
    const uint32_t* q = reinterpret_cast<const uint32_t*>(p);
#pragma unroll
    for (int j = 0; j < 12; ++j) r.w[11 - j] = __builtin_bswap32(q[j]);
  } else {
#pragma unroll
    for (int j = 0; j < 12; ++j)
      r.w[11 - j] = ((uint32_t)p[4 * j] << 24) | ((uint32_t)p[4 * j + 1] << 16) | ((uint32_t)p[4 * j + 2] << 8) | (uint32_t)p[4 * j + 3];
  }
  return r;
}
ECS_DEV void be48_store(uint8_t* __restrict__ p, const fe381& v, uint32_t aligned) {
  if (aligned) {
    uint32_t* q = reinterpret_cast<uint32_t*>(p);
#pragma unroll
    for (int j = 0; j < 12; ++j) q[j] = __builtin_bswap32(v.w[11 - j]);
  } else {
#pragma unroll
    for (int j = 0; j < 12; ++j) {
      const uint32_t w = v.w[11 - j];
      p[4 * j] = (uint8_t)(w >> 24); p[4 * j + 1] = (uint8_t)(w >> 16); p[4 * j + 2] = (uint8_t)(w >> 8); p[4 * j + 3] = (uint8_t)w;
    }
  }
}
// ---- workspace arrays
ECS_DEV fe381 ws_load(const uint64_t* __restrict__ a, size_t e) {
  const uint4* p = reinterpret_cast<const uint4*>(a) + 3 * e;
  const uint4 q0 = p[0], q1 = p[1], q2 = p[2];
  fe381 r;
  r.w[0] = q0.x; r.w[1] = q0.y; r.w[2] = q0.z; r.w[3] = q0.w; r.w[4] = q1.x; r.w[5] = q1.y; r.w[6] = q1.z; r.w[7] = q1.w; r.w[8] = q2.x; r.w[9] = q2.y; r.w[10] = q2.z; r.w[11] = q2.w;
  return r;
}
ECS_DEV void ws_store(uint64_t* __restrict__ a, size_t e, const fe381& v) {
  uint4* p = reinterpret_cast<uint4*>(a) + 3 * e;
  p[0] = make_uint4(v.w[0], v.w[1], v.w[2], v.w[3]); p[1] = make_uint4(v.w[4], v.w[5], v.w[6], v.w[7]); p[2] = make_uint4(v.w[8], v.w[9], v.w[10], v.w[11]);
}
ECS_DEV fe fe_zero8() {
  fe r;
#pragma unroll
  for (int j = 0; j < 8; ++j) r.w[j] = 0u;
  return r;
}
}  // namespace ecsimd_hip
