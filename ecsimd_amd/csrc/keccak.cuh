// keccak.cuh -- Keccak-f[1600] with one state per lane, and the Keccak-256 sponge (rate 136, capacity 512) on it.  PUBLIC data only: nothing here takes a secret.
//
// The 25 lanes of 64 bits live in registers (50 VGPRs; the round's second copy B, the column parities C and D come and go around them).  All 24 rounds are
// unrolled, so every lane index and every rho offset is a compile-time value: an array indexed by a loop variable would go to scratch memory, and a rotation
// by a variable count costs three instructions per half where a constant one is a single funnel shift (v_alignbit_b32) per half -- a rotation by 32 would be
// a rename, but no rho offset is 32.  The round constants are literals of the final XOR.  Plain C++ only.  The instruction count of the shipped ISA is in
// DESIGN.md and profiles/r08/keccak_eth.txt.
//
// Bytes enter a lane little-endian, as Keccak reads them: lane j of a block is its bytes 8 j .. 8 j + 7, the first one lowest.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <hip/hip_runtime.h>

namespace ecsimd_hip {

#define KECCAK_DEV __device__ __forceinline__

struct keccak_consts {
  static constexpr uint64_t RC[24] = {
      0x0000000000000001ull, 0x0000000000008082ull, 0x800000000000808aull, 0x8000000080008000ull, 0x000000000000808bull, 0x0000000080000001ull,
      0x8000000080008081ull, 0x8000000000008009ull, 0x000000000000008aull, 0x0000000000000088ull, 0x0000000080008009ull, 0x000000008000000aull,
      0x000000008000808bull, 0x800000000000008bull, 0x8000000000008089ull, 0x8000000000008003ull, 0x8000000000008002ull, 0x8000000000000080ull,
      0x000000000000800aull, 0x800000008000000aull, 0x8000000080008081ull, 0x8000000000008080ull, 0x0000000080000001ull, 0x8000000080008008ull};
  // rho: the rotation of lane (x, y), at index x + 5 y
  static constexpr int RHO[25] = {0, 1, 62, 28, 27, 36, 44, 6, 55, 20, 3, 10, 43, 25, 39, 41, 45, 15, 21, 8, 18, 2, 61, 56, 14};
};
constexpr int KECCAK_RATE = 136;          // bytes per block: 1600 - 2 x 256 bits
constexpr int KECCAK_RATE_LANES = 17, KECCAK_RATE_WORDS = 34;

struct keccak_state { uint64_t a[25]; };

KECCAK_DEV keccak_state keccak_zero() {
  keccak_state s;
#pragma unroll
  for (int i = 0; i < 25; ++i) s.a[i] = 0;
  return s;
}

// x rotated left by the constant n: the two halves are funnel shifts of the halves of x (v_alignbit_b32 each)
KECCAK_DEV uint64_t keccak_rotl(uint64_t x, int n) {
  if (n == 0) return x;
  uint32_t lo = (uint32_t)x, hi = (uint32_t)(x >> 32);
  if (n >= 32) { const uint32_t t = lo; lo = hi; hi = t; n -= 32; }              // by 32: the halves change names
  if (n == 0) return ((uint64_t)hi << 32) | lo;
  const uint32_t nlo = (lo << n) | (hi >> (32 - n)), nhi = (hi << n) | (lo >> (32 - n));
  return ((uint64_t)nhi << 32) | nlo;
}

KECCAK_DEV void keccak_f1600(keccak_state& s) {
#pragma unroll
  for (int round = 0; round < 24; ++round) {
    uint64_t C[5], B[25];
#pragma unroll
    for (int x = 0; x < 5; ++x) C[x] = s.a[x] ^ s.a[x + 5] ^ s.a[x + 10] ^ s.a[x + 15] ^ s.a[x + 20];                    // theta
#pragma unroll
    for (int x = 0; x < 5; ++x) {
      const uint64_t D = C[(x + 4) % 5] ^ keccak_rotl(C[(x + 1) % 5], 1);
#pragma unroll
      for (int y = 0; y < 5; ++y) s.a[x + 5 * y] ^= D;
    }
#pragma unroll
    for (int x = 0; x < 5; ++x)                                                                                            // rho and pi
#pragma unroll
      for (int y = 0; y < 5; ++y) B[y + 5 * ((2 * x + 3 * y) % 5)] = keccak_rotl(s.a[x + 5 * y], keccak_consts::RHO[x + 5 * y]);
#pragma unroll
    for (int y = 0; y < 5; ++y)                                                                                            // chi
#pragma unroll
      for (int x = 0; x < 5; ++x) s.a[x + 5 * y] = B[x + 5 * y] ^ (~B[(x + 1) % 5 + 5 * y] & B[(x + 2) % 5 + 5 * y]);
    s.a[0] ^= keccak_consts::RC[round];                                                                                    // iota
  }
}

// XORs a block given as 34 little-endian words into the rate part of the state
KECCAK_DEV void keccak_xor_words(keccak_state& s, const uint32_t (&w)[KECCAK_RATE_WORDS]) {
#pragma unroll
  for (int j = 0; j < KECCAK_RATE_LANES; ++j) s.a[j] ^= ((uint64_t)w[2 * j + 1] << 32) | w[2 * j];
}

// A whole block of message bytes at q.  ALIGN (8, 4 or 1) divides the address: 8- or 4-byte loads, else byte loads.  (A block is 136 = 8 x 17 bytes: blocks
// of a 16-byte aligned message alternate between 0 and 8 modulo 16, so 8 bytes is the widest load that every block can use.)
template <int ALIGN> KECCAK_DEV void keccak_absorb_block(keccak_state& s, const uint8_t* q) {
  if constexpr (ALIGN == 8) {
    const uint2* w = reinterpret_cast<const uint2*>(q);
#pragma unroll
    for (int j = 0; j < KECCAK_RATE_LANES; ++j) { const uint2 v = w[j]; s.a[j] ^= ((uint64_t)v.y << 32) | v.x; }
  } else {
    uint32_t w[KECCAK_RATE_WORDS];
    if constexpr (ALIGN == 4) {
      const uint32_t* p = reinterpret_cast<const uint32_t*>(q);
#pragma unroll
      for (int k = 0; k < KECCAK_RATE_WORDS; ++k) w[k] = p[k];
    } else {
#pragma unroll
      for (int k = 0; k < KECCAK_RATE_WORDS; ++k) w[k] = (uint32_t)q[4 * k] | ((uint32_t)q[4 * k + 1] << 8) | ((uint32_t)q[4 * k + 2] << 16) | ((uint32_t)q[4 * k + 3] << 24);
    }
    keccak_xor_words(s, w);
  }
}

// a where mask is all ones, b where it is zero -- as arithmetic on the address: written as a select of two pointers the compiler turns the load behind it
// back into a load under a branch, one wait per load
KECCAK_DEV const uint8_t* keccak_pick(uint32_t mask, const uint8_t* a, const uint8_t* b) {
  const uintptr_t ia = reinterpret_cast<uintptr_t>(a), ib = reinterpret_cast<uintptr_t>(b);
  return reinterpret_cast<const uint8_t*>(ib + ((ia - ib) & (uintptr_t)(int64_t)(int32_t)mask));
}

// The last block: the rem (0 .. 135) message bytes at q, the pad byte `pad` (0x01 for Keccak) right behind them, zeros, and bit 7 of byte 135.  No branch:
// a byte or word that lies behind the message is not read -- its load is pointed at `spare` instead (any readable, 4-byte aligned address: the lane's own
// output slot) and the value dropped, so all the loads are in flight together and none of them leaves the message.
template <int ALIGN> KECCAK_DEV void keccak_absorb_last(keccak_state& s, const uint8_t* q, uint32_t rem, uint32_t pad, const uint8_t* spare) {
  uint32_t w[KECCAK_RATE_WORDS];
  const uint32_t whole = rem >> 2, part = rem & 3u;             // words that are message bytes only; bytes of the one that is not
  uint32_t edge = pad << (8 * part);                            // that word: `part` message bytes, then the pad byte
  if constexpr (ALIGN >= 4) {
#pragma unroll
    for (uint32_t t = 0; t < 3; ++t) {
      const uint32_t have = 0u - (uint32_t)(t < part);
      const uint32_t b = *keccak_pick(have, q + 4 * (size_t)whole + t, spare);
      edge |= (b & have) << (8 * t);
    }
#pragma unroll
    for (uint32_t k = 0; k < KECCAK_RATE_WORDS; ++k) {
      const uint32_t have = 0u - (uint32_t)(k < whole);
      w[k] = *reinterpret_cast<const uint32_t*>(keccak_pick(have, q + 4 * k, spare)) & have;
    }
  } else {
#pragma unroll
    for (uint32_t k = 0; k < KECCAK_RATE_WORDS; ++k) {
      uint32_t v = 0;
#pragma unroll
      for (uint32_t t = 0; t < 4; ++t) {
        const uint32_t have = 0u - (uint32_t)(4 * k + t < rem);
        const uint32_t b = *keccak_pick(have, q + 4 * k + t, spare);
        v |= (b & have) << (8 * t);
      }
      w[k] = v;                                                 // (the edge word holds its message bytes already: the pad byte joins them below)
    }
  }
#pragma unroll
  for (uint32_t k = 0; k < KECCAK_RATE_WORDS; ++k) w[k] |= edge & (0u - (uint32_t)(k == whole));
  w[KECCAK_RATE_WORDS - 1] ^= 0x80000000u;
  keccak_xor_words(s, w);
}

}  // namespace ecsimd_hip
