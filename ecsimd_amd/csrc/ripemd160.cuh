// ripemd160.cuh -- RIPEMD-160 (Dobbertin, Bosselaers, Preneel 1996) with one message block per lane, in the style of sha256.cuh.
//
// The compression function keeps its five state words, the two lines' five working words each and the sixteen message words in registers: all 80 + 80 steps
// are unrolled, so every message index and rotation count is a compile-time value (an array indexed by a loop variable would go to scratch memory) and the
// round constants become literals of the additions.  Rotations are funnel shifts of a word with itself (v_alignbit_b32), the five boolean functions
// three-input bit operations (v_bitop3_b32 / v_bfi_b32 on gfx950).  Plain C++ only.  A step is  T = rol(A + f(B, C, D) + X[r] + K, s) + E,  C = rol(C, 10):
// two three-operand additions or their equal, one boolean, two rotations, one addition.
//
// Words are little-endian throughout, as RIPEMD-160 reads them: a message in memory is loaded as it lies, and the digest's 20 bytes are the five state words
// stored as they are.  A SHA-256 digest (big-endian words) entering a block is byte-swapped word by word: HASH160's only swaps.
#pragma once
#include <stdint.h>
#include "sha256.cuh"

namespace ecsimd_hip {

struct rmd160_consts {
  static constexpr uint32_t IV[5] = {0x67452301u, 0xefcdab89u, 0x98badcfeu, 0x10325476u, 0xc3d2e1f0u};
  static constexpr uint32_t KL[5] = {0x00000000u, 0x5a827999u, 0x6ed9eba1u, 0x8f1bbcdcu, 0xa953fd4eu};
  static constexpr uint32_t KR[5] = {0x50a28be6u, 0x5c4dd124u, 0x6d703ef3u, 0x7a6d76e9u, 0x00000000u};
  static constexpr uint8_t RL[80] = {0, 1, 2,  3,  4,  5,  6,  7,  8,  9,  10, 11, 12, 13, 14, 15, 7, 4, 13, 1,  10, 6, 15, 3,  12, 0, 9, 5,  2,  14, 11, 8,  3, 10, 14, 4, 9,  15, 8,  1,
                                     2, 7, 0,  6,  13, 11, 5,  12, 1,  9,  11, 10, 0,  8,  12, 4,  13, 3, 7, 15, 14, 5, 6,  2,  4,  0, 5, 9,  7,  12, 2,  10, 14, 1, 3,  8, 11, 6,  15, 13};
  static constexpr uint8_t RR[80] = {5,  14, 7, 0, 9, 2,  11, 4, 13, 6, 15, 8, 1,  10, 3,  12, 6, 11, 3, 7, 0, 13, 5,  10, 14, 15, 8, 12, 4,  9,  1, 2,  15, 5,  1,  3, 7, 14, 6, 9,
                                     11, 8,  12, 2, 10, 0, 4,  13, 8, 6, 4,  1, 3,  11, 15, 0,  5, 12, 2, 13, 9, 7, 10, 14, 12, 15, 10, 4, 1, 5,  8, 7,  6,  2,  13, 14, 0, 3,  9, 11};
  static constexpr uint8_t SL[80] = {11, 14, 15, 12, 5,  8,  7,  9,  11, 13, 14, 15, 6,  7,  9,  8,  7, 6, 8, 13, 11, 9, 7, 15, 7,  12, 15, 9,  11, 7,  13, 12, 11, 13, 6,  7, 14, 9,  13, 15,
                                     14, 8,  13, 6,  5,  12, 7,  5,  11, 12, 14, 15, 14, 15, 9,  8,  9, 14, 5, 6, 8,  6, 5, 12, 9,  15, 5,  11, 6,  8,  13, 12, 5,  12, 13, 14, 11, 8, 5,  6};
  static constexpr uint8_t SR[80] = {8,  9,  9,  11, 13, 15, 15, 5,  7,  7,  8,  11, 14, 14, 12, 6,  9, 13, 15, 7, 12, 8, 9,  11, 7, 7, 12, 7,  6,  15, 13, 11, 9,  7,  15, 11, 8, 6,  6, 14,
                                     12, 13, 5,  14, 13, 13, 7,  5,  15, 5,  8,  11, 14, 14, 6,  14, 6, 9,  12, 9, 12, 5, 15, 8,  8, 5, 12, 9,  12, 5,  14, 6,  8,  13, 6,  5,  15, 13, 11, 11};
};

struct rmd160_state { uint32_t h[5]; };
struct rmd160_block { uint32_t w[16]; };       // little-endian words

ECS_DEV uint32_t rmd_rotl(uint32_t x, int n) { return (x << n) | (x >> (32 - n)); }                       // v_alignbit_b32 x, x, 32 - n
// the five boolean functions, by round of the left line (the right line takes them in the opposite order); `round` is a literal after unrolling
ECS_DEV uint32_t rmd_f(int round, uint32_t x, uint32_t y, uint32_t z) {
  switch (round) {
    case 0: return x ^ y ^ z;
    case 1: return sha_bfi(x, y, z);                 // (x & y) | (~x & z)
    case 2: return (x | ~y) ^ z;
    case 3: return sha_bfi(z, x, y);                 // (x & z) | (y & ~z)
    default: return x ^ (y | ~z);
  }
}

ECS_DEV rmd160_state rmd160_iv() {
  rmd160_state s;
#pragma unroll
  for (int i = 0; i < 5; ++i) s.h[i] = rmd160_consts::IV[i];
  return s;
}

// one block into the state
ECS_DEV void rmd160_compress(rmd160_state& s, const rmd160_block& m) {
  using K = rmd160_consts;
  uint32_t al = s.h[0], bl = s.h[1], cl = s.h[2], dl = s.h[3], el = s.h[4];
  uint32_t ar = al, br = bl, cr = cl, dr = dl, er = el;
#pragma unroll
  for (int j = 0; j < 80; ++j) {
    const int round = j / 16;
    uint32_t t = rmd_rotl(al + rmd_f(round, bl, cl, dl) + m.w[K::RL[j]] + K::KL[round], K::SL[j]) + el;
    al = el; el = dl; dl = rmd_rotl(cl, 10); cl = bl; bl = t;
    t = rmd_rotl(ar + rmd_f(4 - round, br, cr, dr) + m.w[K::RR[j]] + K::KR[round], K::SR[j]) + er;
    ar = er; er = dr; dr = rmd_rotl(cr, 10); cr = br; br = t;
  }
  const uint32_t t = s.h[1] + cl + dr;
  s.h[1] = s.h[2] + dl + er; s.h[2] = s.h[3] + el + ar; s.h[3] = s.h[4] + al + br; s.h[4] = s.h[0] + bl + cr; s.h[0] = t;
}

// The block of a message's tail at byte offset `base`: its bytes up to msg_bytes, 0x80, zeros, and -- where `last` -- the bit length (little-endian) in the
// last two words.  msg_bytes and base are the same on every lane: every branch here is uniform.
ECS_DEV rmd160_block rmd160_tail_block(const uint8_t* __restrict__ p, size_t msg_bytes, size_t base, bool last) {
  rmd160_block m;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    uint32_t w = 0;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const size_t q = base + 4 * j + t;
      uint32_t byte = 0;
      if (q < msg_bytes) byte = p[q];
      else if (q == msg_bytes) byte = 0x80u;
      w |= byte << (8 * t);
    }
    m.w[j] = w;
  }
  if (last) {
    const uint64_t bits = (uint64_t)msg_bytes * 8u;
    m.w[14] = (uint32_t)bits;
    m.w[15] = (uint32_t)(bits >> 32);
  }
  return m;
}

// The msg_bytes bytes at p, the padding and the bit length.  msg_bytes is the same on every lane; ALIGNED: p and the stride between the lanes' messages are
// multiples of 4 (word loads, no byte swap: the words are little-endian).  Whole blocks go through THE loop of this function; the last one or two blocks --
// two where fewer than 9 bytes are free behind the message -- are padded in registers.
template <bool ALIGNED> ECS_DEV void rmd160_absorb_message(rmd160_state& s, const uint8_t* __restrict__ p, size_t msg_bytes) {
  const size_t full = msg_bytes / 64;
#pragma unroll 1
  for (size_t b = 0; b < full; ++b) {
    rmd160_block m;
    if constexpr (ALIGNED) {
      const uint32_t* q = reinterpret_cast<const uint32_t*>(p + 64 * b);
#pragma unroll
      for (int j = 0; j < 16; ++j) m.w[j] = q[j];
    } else {
      const uint8_t* q = p + 64 * b;
#pragma unroll
      for (int j = 0; j < 16; ++j) m.w[j] = (uint32_t)q[4 * j] | ((uint32_t)q[4 * j + 1] << 8) | ((uint32_t)q[4 * j + 2] << 16) | ((uint32_t)q[4 * j + 3] << 24);
    }
    rmd160_compress(s, m);
  }
  const bool two = msg_bytes - 64 * full >= 56;
  rmd160_compress(s, rmd160_tail_block(p, msg_bytes, 64 * full, !two));
  if (two) rmd160_compress(s, rmd160_tail_block(p, msg_bytes, 64 * full + 64, true));
}

// The same for a length of the lane's own (PUBLIC: the loop's trip count is the lane's), in the shape of sha256_absorb_message_lens: len / 64 whole blocks, the
// tail block from msg_tail_words_le -- no byte at or behind p + len is loaded, `spare` takes those loads --, a block of zeros behind it where fewer than 9
// bytes are free, the bit length (little-endian) in the last.
template <bool ALIGNED> ECS_DEV void rmd160_absorb_message_lens(rmd160_state& s, const uint8_t* p, uint32_t len, const uint8_t* spare) {
  const uint32_t full = len >> 6, rem = len & 63u;
  rmd160_block m;
#pragma unroll 1
  for (uint32_t b = 0; b < full; ++b) {
    msg_words_le<ALIGNED>(p, m.w);
    rmd160_compress(s, m);
    p += 64;
  }
  msg_tail_words_le<ALIGNED>(p, rem, spare, m.w);
  const uint32_t tails = rem >= 56u ? 2u : 1u;
#pragma unroll 1
  for (uint32_t t = 0; t < tails; ++t) {
    if (t + 1 == tails) { m.w[14] = len << 3; m.w[15] = len >> 29; }
    rmd160_compress(s, m);
#pragma unroll
    for (int j = 0; j < 16; ++j) m.w[j] = 0u;
  }
}

// RIPEMD160 of a 32-byte SHA-256 digest, straight from the state: one compression (HASH160's second half)
ECS_DEV rmd160_state rmd160_of_sha256(const sha256_state& d) {
  rmd160_block m;
#pragma unroll
  for (int j = 0; j < 8; ++j) m.w[j] = __builtin_bswap32(d.h[j]);
  m.w[8] = 0x80u;
#pragma unroll
  for (int j = 9; j < 16; ++j) m.w[j] = 0u;
  m.w[14] = 256u;
  rmd160_state s = rmd160_iv();
  rmd160_compress(s, m);
  return s;
}
// the digest's 20 bytes at out (4-byte aligned): the state words as they are
ECS_DEV void rmd160_store(uint32_t* __restrict__ out, const rmd160_state& s) {
#pragma unroll
  for (int j = 0; j < 5; ++j) out[j] = s.h[j];
}

}  // namespace ecsimd_hip
