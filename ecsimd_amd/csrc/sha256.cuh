// sha256.cuh -- SHA-256 (FIPS 180-4) with one message block per lane, and the HMAC-SHA-256 shapes RFC 6979 needs on top of it.
//
// The compression function keeps its eight state words and the sixteen-word rolling schedule in registers: all 64 rounds are unrolled, so every schedule
// index is a compile-time value (an array indexed by a loop variable would go to scratch memory) and the round constants become literals of the additions.
// Rotations are written as funnel shifts of a word with itself (v_alignbit_b32), Ch and Maj as bit selects (Ch(e, f, g) = bfi(e, f, g),
// Maj(a, b, c) = bfi(a ^ b, c, b): v_bfi_b32 forms, which gfx950 issues as one three-input v_bitop3_b32 each).  Plain C++ only.  The shipped ISA has about
// 1 500 VALU instructions per compression.
//
// Words are big-endian throughout, as SHA-256 reads them: a 256-bit integer held as eight little-endian 32-bit words w[0..7] (struct fe) enters a block
// as w[7], w[6], ..., w[0] and a digest H0..H7 IS the integer with w[7 - j] = Hj -- no byte swap anywhere.
#pragma once
#include <stdint.h>
#include "field.cuh"

namespace ecsimd_hip {

struct sha256_consts {
  static constexpr uint32_t K[64] = {
      0x428a2f98u, 0x71374491u, 0xb5c0fbcfu, 0xe9b5dba5u, 0x3956c25bu, 0x59f111f1u, 0x923f82a4u, 0xab1c5ed5u, 0xd807aa98u, 0x12835b01u, 0x243185beu, 0x550c7dc3u,
      0x72be5d74u, 0x80deb1feu, 0x9bdc06a7u, 0xc19bf174u, 0xe49b69c1u, 0xefbe4786u, 0x0fc19dc6u, 0x240ca1ccu, 0x2de92c6fu, 0x4a7484aau, 0x5cb0a9dcu, 0x76f988dau,
      0x983e5152u, 0xa831c66du, 0xb00327c8u, 0xbf597fc7u, 0xc6e00bf3u, 0xd5a79147u, 0x06ca6351u, 0x14292967u, 0x27b70a85u, 0x2e1b2138u, 0x4d2c6dfcu, 0x53380d13u,
      0x650a7354u, 0x766a0abbu, 0x81c2c92eu, 0x92722c85u, 0xa2bfe8a1u, 0xa81a664bu, 0xc24b8b70u, 0xc76c51a3u, 0xd192e819u, 0xd6990624u, 0xf40e3585u, 0x106aa070u,
      0x19a4c116u, 0x1e376c08u, 0x2748774cu, 0x34b0bcb5u, 0x391c0cb3u, 0x4ed8aa4au, 0x5b9cca4fu, 0x682e6ff3u, 0x748f82eeu, 0x78a5636fu, 0x84c87814u, 0x8cc70208u,
      0x90befffau, 0xa4506cebu, 0xbef9a3f7u, 0xc67178f2u};
  static constexpr uint32_t IV[8] = {0x6a09e667u, 0xbb67ae85u, 0x3c6ef372u, 0xa54ff53au, 0x510e527fu, 0x9b05688cu, 0x1f83d9abu, 0x5be0cd19u};
};

struct sha256_state { uint32_t h[8]; };
struct sha256_block { uint32_t w[16]; };

ECS_DEV uint32_t sha_rotr(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }                     // v_alignbit_b32 x, x, n
ECS_DEV uint32_t sha_bfi(uint32_t m, uint32_t a, uint32_t b) { return b ^ (m & (a ^ b)); }              // m ? a : b bit by bit

ECS_DEV sha256_state sha256_iv() {
  sha256_state s;
#pragma unroll
  for (int i = 0; i < 8; ++i) s.h[i] = sha256_consts::IV[i];
  return s;
}

// one block into the state; the block is taken by value (the schedule rolls over it)
ECS_DEV void sha256_compress(sha256_state& s, sha256_block m) {
  uint32_t a = s.h[0], b = s.h[1], c = s.h[2], d = s.h[3], e = s.h[4], f = s.h[5], g = s.h[6], h = s.h[7];
#pragma unroll
  for (int t = 0; t < 64; ++t) {
    if (t >= 16) {
      const uint32_t w15 = m.w[(t - 15) & 15], w2 = m.w[(t - 2) & 15];
      const uint32_t s0 = sha_rotr(w15, 7) ^ sha_rotr(w15, 18) ^ (w15 >> 3);
      const uint32_t s1 = sha_rotr(w2, 17) ^ sha_rotr(w2, 19) ^ (w2 >> 10);
      m.w[t & 15] += s0 + m.w[(t - 7) & 15] + s1;
    }
    const uint32_t S1 = sha_rotr(e, 6) ^ sha_rotr(e, 11) ^ sha_rotr(e, 25);
    const uint32_t S0 = sha_rotr(a, 2) ^ sha_rotr(a, 13) ^ sha_rotr(a, 22);
    const uint32_t t1 = h + S1 + sha_bfi(e, f, g) + sha256_consts::K[t] + m.w[t & 15];
    const uint32_t t2 = S0 + sha_bfi(a ^ b, c, b);
    h = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + t2;
  }
  s.h[0] += a; s.h[1] += b; s.h[2] += c; s.h[3] += d; s.h[4] += e; s.h[5] += f; s.h[6] += g; s.h[7] += h;
}

// The rest of a hash whose first prefix_bytes bytes (a multiple of 64) are in the state already: the msg_bytes bytes at p, the padding and the bit length
// of the whole.  msg_bytes, prefix_bytes and `aligned` (p and the stride between the lanes' messages are multiples of 4: word loads) are the same on every
// lane, so every branch here is uniform; the last one or two blocks are padded in registers.
ECS_DEV void sha256_absorb_message(sha256_state& s, const uint8_t* __restrict__ p, size_t msg_bytes, uint32_t aligned, size_t prefix_bytes) {
  const size_t blocks = (msg_bytes + 9 + 63) / 64;
  const uint64_t bits = ((uint64_t)prefix_bytes + (uint64_t)msg_bytes) * 8u;
#pragma unroll 1
  for (size_t b = 0; b < blocks; ++b) {
    const size_t base = 64 * b;
    sha256_block m;
    if (base + 64 <= msg_bytes) {
      if (aligned) {
        const uint32_t* q = reinterpret_cast<const uint32_t*>(p + base);
#pragma unroll
        for (int j = 0; j < 16; ++j) m.w[j] = __builtin_bswap32(q[j]);
      } else {
#pragma unroll
        for (int j = 0; j < 16; ++j)
          m.w[j] = ((uint32_t)p[base + 4 * j] << 24) | ((uint32_t)p[base + 4 * j + 1] << 16) | ((uint32_t)p[base + 4 * j + 2] << 8) | (uint32_t)p[base + 4 * j + 3];
      }
    } else {                                                   // the message ends in or before this block: its bytes, 0x80, zeros, and the bit length at the very end
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        uint32_t w = 0;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const size_t q = base + 4 * j + t;
          uint32_t byte = 0;
          if (q < msg_bytes) byte = p[q];
          else if (q == msg_bytes) byte = 0x80u;
          w = (w << 8) | byte;
        }
        m.w[j] = w;
      }
      if (b + 1 == blocks) {
        m.w[14] = (uint32_t)(bits >> 32);
        m.w[15] = (uint32_t)bits;
      }
    }
    sha256_compress(s, m);
  }
}

// ---- one length per lane.  PUBLIC lengths: the block loop's trip count and the shape of the tail are the lane's own, so a wave runs until its longest lane
// is done.  ALIGNED as above, a template argument here.
// a where mask is all ones, b where it is zero -- as arithmetic on the address (keccak.cuh's keccak_pick says why)
ECS_DEV const uint8_t* msg_pick(uint32_t mask, const uint8_t* a, const uint8_t* b) {
  const uintptr_t ia = reinterpret_cast<uintptr_t>(a), ib = reinterpret_cast<uintptr_t>(b);
  return reinterpret_cast<const uint8_t*>(ib + ((ia - ib) & (uintptr_t)(int64_t)(int32_t)mask));
}
// the 64 message bytes at q as sixteen little-endian words
template <bool ALIGNED> ECS_DEV void msg_words_le(const uint8_t* q, uint32_t (&w)[16]) {
  if constexpr (ALIGNED) {
    const uint32_t* p = reinterpret_cast<const uint32_t*>(q);
#pragma unroll
    for (int j = 0; j < 16; ++j) w[j] = p[j];
  } else {
#pragma unroll
    for (int j = 0; j < 16; ++j) w[j] = (uint32_t)q[4 * j] | ((uint32_t)q[4 * j + 1] << 8) | ((uint32_t)q[4 * j + 2] << 16) | ((uint32_t)q[4 * j + 3] << 24);
  }
}
// The last rem (0 .. 63) message bytes at q as little-endian words, the byte 0x80 right behind them, zeros.  No branch, and no byte at or behind q + rem is
// loaded (a row's tail need not be allocated): such a load is pointed at `spare` instead -- any readable, 4-byte aligned address: the lane's own output slot --
// and its value dropped, as in keccak_absorb_last.
template <bool ALIGNED> ECS_DEV void msg_tail_words_le(const uint8_t* q, uint32_t rem, const uint8_t* spare, uint32_t (&w)[16]) {
  const uint32_t whole = rem >> 2, part = rem & 3u;            // words that are message bytes only; bytes of the one that is not
  uint32_t edge = 0x80u << (8 * part);                         // that word: `part` message bytes, then the padding's first byte
  if constexpr (ALIGNED) {
#pragma unroll
    for (uint32_t t = 0; t < 3; ++t) {
      const uint32_t have = 0u - (uint32_t)(t < part);
      const uint32_t b = *msg_pick(have, q + 4 * whole + t, spare);
      edge |= (b & have) << (8 * t);
    }
#pragma unroll
    for (uint32_t k = 0; k < 16; ++k) {
      const uint32_t have = 0u - (uint32_t)(k < whole);
      w[k] = *reinterpret_cast<const uint32_t*>(msg_pick(have, q + 4 * k, spare)) & have;
    }
  } else {
#pragma unroll
    for (uint32_t k = 0; k < 16; ++k) {
      uint32_t v = 0;
#pragma unroll
      for (uint32_t t = 0; t < 4; ++t) {
        const uint32_t have = 0u - (uint32_t)(4 * k + t < rem);
        const uint32_t b = *msg_pick(have, q + 4 * k + t, spare);
        v |= (b & have) << (8 * t);
      }
      w[k] = v;                                                // (the edge word holds its message bytes already: the 0x80 joins them below)
    }
  }
#pragma unroll
  for (uint32_t k = 0; k < 16; ++k) w[k] |= edge & (0u - (uint32_t)(k == whole));
}
template <bool ALIGNED> ECS_DEV sha256_block sha256_load_block(const uint8_t* q) {
  uint32_t w[16];
  msg_words_le<ALIGNED>(q, w);
  sha256_block m;
#pragma unroll
  for (int j = 0; j < 16; ++j) m.w[j] = __builtin_bswap32(w[j]);
  return m;
}
template <bool ALIGNED> ECS_DEV sha256_block sha256_load_tail(const uint8_t* q, uint32_t rem, const uint8_t* spare) {
  uint32_t w[16];
  msg_tail_words_le<ALIGNED>(q, rem, spare, w);
  sha256_block m;
#pragma unroll
  for (int j = 0; j < 16; ++j) m.w[j] = __builtin_bswap32(w[j]);
  return m;
}
// sha256_absorb_message for a length of the lane's own: the len bytes at p, the padding and the bit length.  Whole blocks go through THE loop of this function,
// len / 64 trips; the tail block comes from sha256_load_tail, and where fewer than 9 bytes are free behind the message a block of zeros follows it: the
// second loop's one or two trips, the bit length in the last.
template <bool ALIGNED> ECS_DEV void sha256_absorb_message_lens(sha256_state& s, const uint8_t* p, uint32_t len, const uint8_t* spare) {
  const uint32_t full = len >> 6, rem = len & 63u;
#pragma unroll 1
  for (uint32_t b = 0; b < full; ++b) {
    sha256_compress(s, sha256_load_block<ALIGNED>(p));
    p += 64;
  }
  sha256_block m = sha256_load_tail<ALIGNED>(p, rem, spare);
  const uint32_t tails = rem >= 56u ? 2u : 1u;
#pragma unroll 1
  for (uint32_t t = 0; t < tails; ++t) {
    if (t + 1 == tails) { m.w[14] = len >> 29; m.w[15] = len << 3; }
    sha256_compress(s, m);
#pragma unroll
    for (int j = 0; j < 16; ++j) m.w[j] = 0u;
  }
}

// ---- 256-bit integers <-> big-endian words
ECS_DEV void sha_words_of(const fe& x, uint32_t (&be)[8]) {
#pragma unroll
  for (int j = 0; j < 8; ++j) be[j] = x.w[7 - j];
}
ECS_DEV fe sha_digest_fe(const sha256_state& s) {
  fe r;
#pragma unroll
  for (int j = 0; j < 8; ++j) r.w[7 - j] = s.h[j];
  return r;
}

// ---- HMAC-SHA-256 with a 32-byte key, as two midstates: the state after the key's ipad block and after its opad block.  Every HMAC under one key starts
// from them instead of compressing the key again.
struct hmac_key { sha256_state inner, outer; };

ECS_DEV hmac_key hmac_key_from(const sha256_state& key) {              // key = 32 bytes as eight big-endian words, zero-padded to the block
  sha256_block bi, bo;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const uint32_t kw = j < 8 ? key.h[j] : 0u;
    bi.w[j] = kw ^ 0x36363636u;
    bo.w[j] = kw ^ 0x5c5c5c5cu;
  }
  hmac_key k;
  k.inner = sha256_iv(); sha256_compress(k.inner, bi);
  k.outer = sha256_iv(); sha256_compress(k.outer, bo);
  return k;
}
// the last block of a hash of total_bytes bytes whose final 32 (or 33) are v (and a zero byte): v, after_word, zeros, the bit length
ECS_DEV sha256_block sha_tail_block32(const sha256_state& v, uint32_t after_word, uint32_t total_bytes) {
  sha256_block b;
#pragma unroll
  for (int j = 0; j < 8; ++j) b.w[j] = v.h[j];
  b.w[8] = after_word;                                                  // 0x80000000: the padding bit right behind v; 0x00800000: a zero byte, then the bit
#pragma unroll
  for (int j = 9; j < 15; ++j) b.w[j] = 0u;
  b.w[15] = total_bytes * 8u;
  return b;
}
// the outer hash: H(opad block || inner digest)
ECS_DEV sha256_state hmac_finish(const hmac_key& k, const sha256_state& inner) {
  sha256_state o = k.outer;
  sha256_compress(o, sha_tail_block32(inner, 0x80000000u, 96u));
  return o;
}
// HMAC_K(v), v = 32 bytes: two compressions
ECS_DEV sha256_state hmac32(const hmac_key& k, const sha256_state& v) {
  sha256_state in = k.inner;
  sha256_compress(in, sha_tail_block32(v, 0x80000000u, 96u));
  return hmac_finish(k, in);
}
// HMAC_K(v || 0x00): RFC 6979 3.2 h.3's key update; two compressions
ECS_DEV sha256_state hmac32_zero(const hmac_key& k, const sha256_state& v) {
  sha256_state in = k.inner;
  sha256_compress(in, sha_tail_block32(v, 0x00800000u, 97u));
  return hmac_finish(k, in);
}
// HMAC_K(v || sep || x || h), 97 bytes (RFC 6979 3.2 d and f; sep = 0x00 / 0x01; x, h = eight big-endian words each): three compressions.
// The byte `sep` shifts x and h by one byte against the word grid: every word behind it is a funnel shift of two neighbours.
ECS_DEV sha256_state hmac97(const hmac_key& k, const sha256_state& v, uint32_t sep, const uint32_t (&x)[8], const uint32_t (&h)[8]) {
  auto join = [](uint32_t hi, uint32_t lo) { return (hi << 24) | (lo >> 8); };
  sha256_block a, b;
#pragma unroll
  for (int j = 0; j < 8; ++j) a.w[j] = v.h[j];
  a.w[8] = join(sep, x[0]);
#pragma unroll
  for (int j = 1; j < 8; ++j) a.w[8 + j] = join(x[j - 1], x[j]);
  b.w[0] = join(x[7], h[0]);
#pragma unroll
  for (int j = 1; j < 8; ++j) b.w[j] = join(h[j - 1], h[j]);
  b.w[8] = (h[7] << 24) | 0x00800000u;
#pragma unroll
  for (int j = 9; j < 15; ++j) b.w[j] = 0u;
  b.w[15] = (64u + 97u) * 8u;
  sha256_state in = k.inner;
  sha256_compress(in, a);
  sha256_compress(in, b);
  return hmac_finish(k, in);
}

}  // namespace ecsimd_hip
