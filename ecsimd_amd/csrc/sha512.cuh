// sha512.cuh -- SHA-512 (FIPS 180-4) with one message block per lane, and the two tail blocks HMAC-SHA-512 needs on top of it.
//
// The shape of sha256.cuh: eight state words and the sixteen-word rolling schedule in registers, all 80 rounds unrolled, so every schedule index is a
// compile-time value (nothing goes to scratch memory) and the round constants are literals.  gfx950's VALU is 32 bits wide, so a 64-bit word is a register
// pair and what the compiler makes of plain uint64_t matters:
//   * an addition is ONE instruction (v_lshl_add_u64), so additions stay 64-bit;
//   * a rotation written (x >> n) | (x << (64 - n)) becomes two 64-bit shifts and two ORs.  Here it is written on the halves instead, as keccak.cuh's: each
//     half of the result is a funnel shift of the two halves of x (v_alignbit_b32), with the halves changing names for n >= 32.  A right shift is one
//     funnel shift and one 32-bit shift;
//   * Ch and Maj are bit selects per half (sha256.cuh's sha_bfi: one three-input v_bitop3_b32 each).
// Plain C++ only.  DESIGN.md section 4c has the instruction counts of the shipped ISA beside those of the same function written on uint64_t.
//
// Words are big-endian, as SHA-512 reads them: a 256-bit integer held as eight little-endian 32-bit words w[0..7] (struct fe) is the four block words
// (w[7] : w[6]), (w[5] : w[4]), (w[3] : w[2]), (w[1] : w[0]); a digest H0..H7 is two such integers, H0..H3 and H4..H7 -- no byte swap anywhere.
#pragma once
#include <stdint.h>
#include "field.cuh"
#include "sha256.cuh"

namespace ecsimd_hip {

struct sha512_consts {
  static constexpr uint64_t K[80] = {
      0x428a2f98d728ae22ull, 0x7137449123ef65cdull, 0xb5c0fbcfec4d3b2full, 0xe9b5dba58189dbbcull,
      0x3956c25bf348b538ull, 0x59f111f1b605d019ull, 0x923f82a4af194f9bull, 0xab1c5ed5da6d8118ull,
      0xd807aa98a3030242ull, 0x12835b0145706fbeull, 0x243185be4ee4b28cull, 0x550c7dc3d5ffb4e2ull,
      0x72be5d74f27b896full, 0x80deb1fe3b1696b1ull, 0x9bdc06a725c71235ull, 0xc19bf174cf692694ull,
      0xe49b69c19ef14ad2ull, 0xefbe4786384f25e3ull, 0x0fc19dc68b8cd5b5ull, 0x240ca1cc77ac9c65ull,
      0x2de92c6f592b0275ull, 0x4a7484aa6ea6e483ull, 0x5cb0a9dcbd41fbd4ull, 0x76f988da831153b5ull,
      0x983e5152ee66dfabull, 0xa831c66d2db43210ull, 0xb00327c898fb213full, 0xbf597fc7beef0ee4ull,
      0xc6e00bf33da88fc2ull, 0xd5a79147930aa725ull, 0x06ca6351e003826full, 0x142929670a0e6e70ull,
      0x27b70a8546d22ffcull, 0x2e1b21385c26c926ull, 0x4d2c6dfc5ac42aedull, 0x53380d139d95b3dfull,
      0x650a73548baf63deull, 0x766a0abb3c77b2a8ull, 0x81c2c92e47edaee6ull, 0x92722c851482353bull,
      0xa2bfe8a14cf10364ull, 0xa81a664bbc423001ull, 0xc24b8b70d0f89791ull, 0xc76c51a30654be30ull,
      0xd192e819d6ef5218ull, 0xd69906245565a910ull, 0xf40e35855771202aull, 0x106aa07032bbd1b8ull,
      0x19a4c116b8d2d0c8ull, 0x1e376c085141ab53ull, 0x2748774cdf8eeb99ull, 0x34b0bcb5e19b48a8ull,
      0x391c0cb3c5c95a63ull, 0x4ed8aa4ae3418acbull, 0x5b9cca4f7763e373ull, 0x682e6ff3d6b2b8a3ull,
      0x748f82ee5defb2fcull, 0x78a5636f43172f60ull, 0x84c87814a1f0ab72ull, 0x8cc702081a6439ecull,
      0x90befffa23631e28ull, 0xa4506cebde82bde9ull, 0xbef9a3f7b2c67915ull, 0xc67178f2e372532bull,
      0xca273eceea26619cull, 0xd186b8c721c0c207ull, 0xeada7dd6cde0eb1eull, 0xf57d4f7fee6ed178ull,
      0x06f067aa72176fbaull, 0x0a637dc5a2c898a6ull, 0x113f9804bef90daeull, 0x1b710b35131c471bull,
      0x28db77f523047d84ull, 0x32caab7b40c72493ull, 0x3c9ebe0a15c9bebcull, 0x431d67c49c100d4cull,
      0x4cc5d4becb3e42b6ull, 0x597f299cfc657e2aull, 0x5fcb6fab3ad6faecull, 0x6c44198c4a475817ull};
  static constexpr uint64_t IV[8] = {0x6a09e667f3bcc908ull, 0xbb67ae8584caa73bull, 0x3c6ef372fe94f82bull, 0xa54ff53a5f1d36f1ull,
                                     0x510e527fade682d1ull, 0x9b05688c2b3e6c1full, 0x1f83d9abfb41bd6bull, 0x5be0cd19137e2179ull};
};

struct sha512_state { uint64_t h[8]; };
struct sha512_block { uint64_t w[16]; };

ECS_DEV uint64_t sha512_join(uint32_t hi, uint32_t lo) { return ((uint64_t)hi << 32) | lo; }
// x rotated right by the constant n (0 < n < 64, n != 32): two funnel shifts of the halves of x
ECS_DEV uint64_t sha512_rotr(uint64_t x, int n) {
  uint32_t lo = (uint32_t)x, hi = (uint32_t)(x >> 32);
  if (n >= 32) { const uint32_t t = lo; lo = hi; hi = t; n -= 32; }                // by 32: the halves change names
  return sha512_join((hi >> n) | (lo << (32 - n)), (lo >> n) | (hi << (32 - n)));
}
// x >> n (0 < n < 32): one funnel shift and one shift
ECS_DEV uint64_t sha512_shr(uint64_t x, int n) {
  const uint32_t lo = (uint32_t)x, hi = (uint32_t)(x >> 32);
  return sha512_join(hi >> n, (lo >> n) | (hi << (32 - n)));
}
// m ? a : b bit by bit, per half
ECS_DEV uint64_t sha512_bfi(uint64_t m, uint64_t a, uint64_t b) {
  return sha512_join(sha_bfi((uint32_t)(m >> 32), (uint32_t)(a >> 32), (uint32_t)(b >> 32)), sha_bfi((uint32_t)m, (uint32_t)a, (uint32_t)b));
}

ECS_DEV sha512_state sha512_iv() {
  sha512_state s;
#pragma unroll
  for (int i = 0; i < 8; ++i) s.h[i] = sha512_consts::IV[i];
  return s;
}

// Rounds T .. 79.  The unrolling is spelled out as a recursion over the round number: eighty rounds on split halves are more than the compiler unrolls at a
// pragma's request, and a loop left standing would index the schedule with a variable -- scratch memory.  The working variables do not move: round T's
// a .. h are v[(0 - T) & 7] .. v[(7 - T) & 7].
template <int T> ECS_DEV void sha512_rounds(uint64_t (&v)[8], sha512_block& m) {
  if constexpr (T < 80) {
    if constexpr (T >= 16) {
      const uint64_t w15 = m.w[(T - 15) & 15], w2 = m.w[(T - 2) & 15];
      const uint64_t s0 = sha512_rotr(w15, 1) ^ sha512_rotr(w15, 8) ^ sha512_shr(w15, 7);
      const uint64_t s1 = sha512_rotr(w2, 19) ^ sha512_rotr(w2, 61) ^ sha512_shr(w2, 6);
      m.w[T & 15] += s0 + m.w[(T - 7) & 15] + s1;
    }
    const uint64_t a = v[(0 - T) & 7], b = v[(1 - T) & 7], c = v[(2 - T) & 7], e = v[(4 - T) & 7], f = v[(5 - T) & 7], g = v[(6 - T) & 7];
    const uint64_t S1 = sha512_rotr(e, 14) ^ sha512_rotr(e, 18) ^ sha512_rotr(e, 41);
    const uint64_t S0 = sha512_rotr(a, 28) ^ sha512_rotr(a, 34) ^ sha512_rotr(a, 39);
    const uint64_t t1 = v[(7 - T) & 7] + S1 + sha512_bfi(e, f, g) + sha512_consts::K[T] + m.w[T & 15];
    const uint64_t t2 = S0 + sha512_bfi(a ^ b, c, b);
    v[(3 - T) & 7] += t1;                                                            // the next round's e
    v[(7 - T) & 7] = t1 + t2;                                                        // the next round's a
    sha512_rounds<T + 1>(v, m);
  }
}
// one block into the state; the block is taken by value (the schedule rolls over it)
ECS_DEV void sha512_compress(sha512_state& s, sha512_block m) {
  uint64_t v[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] = s.h[j];
  sha512_rounds<0>(v, m);
#pragma unroll
  for (int j = 0; j < 8; ++j) s.h[j] += v[j];                                        // 80 rounds: the variables are back in their places
}

// The rest of a hash whose first prefix_bytes bytes (a multiple of 128) are in the state already: the msg_bytes bytes at p, the padding and the bit length
// of the whole (128 bits, the high 64 of them zero).  msg_bytes, prefix_bytes and ALIGNED (p and the stride between the lanes' messages are multiples of 4:
// word loads) are the same on every lane, so every branch here is uniform; the last one or two blocks are padded in registers.
template <bool ALIGNED>
ECS_DEV void sha512_absorb_message(sha512_state& s, const uint8_t* __restrict__ p, size_t msg_bytes, size_t prefix_bytes) {
  const size_t blocks = (msg_bytes + 17 + 127) / 128;
  const uint64_t bits = ((uint64_t)prefix_bytes + (uint64_t)msg_bytes) * 8u;
#pragma unroll 1
  for (size_t b = 0; b < blocks; ++b) {
    const size_t base = 128 * b;
    sha512_block m;
    if (base + 128 <= msg_bytes) {
      if constexpr (ALIGNED) {
        const uint32_t* q = reinterpret_cast<const uint32_t*>(p + base);
#pragma unroll
        for (int j = 0; j < 16; ++j) m.w[j] = sha512_join(__builtin_bswap32(q[2 * j]), __builtin_bswap32(q[2 * j + 1]));
      } else {
#pragma unroll
        for (int j = 0; j < 16; ++j) {
          uint64_t w = 0;
#pragma unroll
          for (int t = 0; t < 8; ++t) w = (w << 8) | (uint64_t)p[base + 8 * j + t];
          m.w[j] = w;
        }
      }
    } else {                                                   // the message ends in or before this block: its bytes, 0x80, zeros, and the bit length at the very end
      const size_t left = msg_bytes > base ? msg_bytes - base : 0;        // message bytes in this block: 0 .. 127
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        uint64_t w = 0;
        if ((size_t)(8 * j + 8) <= left) {                                  // a whole word of message
          if constexpr (ALIGNED) {
            const uint32_t* q = reinterpret_cast<const uint32_t*>(p + base);
            w = sha512_join(__builtin_bswap32(q[2 * j]), __builtin_bswap32(q[2 * j + 1]));
          } else {
#pragma unroll
            for (int t = 0; t < 8; ++t) w = (w << 8) | (uint64_t)p[base + 8 * j + t];
          }
        } else if (msg_bytes >= base && (size_t)(8 * j) <= left) {          // the word the message ends in (or right in front of): up to 7 bytes and 0x80
#pragma unroll
          for (int t = 0; t < 8; ++t) {
            const size_t q = 8 * j + t;
            uint64_t byte = 0;
            if (q < left) byte = p[base + q];
            else if (q == left) byte = 0x80u;
            w = (w << 8) | byte;
          }
        }
        m.w[j] = w;
      }
      if (b + 1 == blocks) {
        m.w[14] = 0u;
        m.w[15] = bits;
      }
    }
    sha512_compress(s, m);
  }
}

// ---- 256-bit integers <-> big-endian 64-bit words
ECS_DEV void sha512_words_of(const fe& x, uint64_t (&be)[4]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) be[j] = sha512_join(x.w[7 - 2 * j], x.w[6 - 2 * j]);
}
// the integer of the digest's words first .. first + 3 (0: the left half, 4: the right half)
ECS_DEV fe sha512_digest_fe(const sha512_state& s, int first) {
  fe r;
#pragma unroll
  for (int j = 0; j < 4; ++j) { r.w[7 - 2 * j] = (uint32_t)(s.h[first + j] >> 32); r.w[6 - 2 * j] = (uint32_t)s.h[first + j]; }
  return r;
}

// ---- the two tail blocks of HMAC-SHA-512
// the last block of a hash of total_bytes bytes whose final 64 are the digest v: v, the padding bit, zeros, the bit length
ECS_DEV sha512_block sha512_tail_block64(const sha512_state& v, uint32_t total_bytes) {
  sha512_block b;
#pragma unroll
  for (int j = 0; j < 8; ++j) b.w[j] = v.h[j];
  b.w[8] = 0x8000000000000000ull;
#pragma unroll
  for (int j = 9; j < 15; ++j) b.w[j] = 0u;
  b.w[15] = (uint64_t)total_bytes * 8u;
  return b;
}
// the one block behind a key block: data_bytes <= 64 bytes of data in d (big-endian words, zero behind the data), the padding bit, zeros, the bit length of
// 128 + data_bytes bytes.  data_bytes is uniform; with a constant one the padding word folds into d's.
ECS_DEV sha512_block sha512_tail_block_short(const uint64_t (&d)[8], uint32_t data_bytes) {
  sha512_block b;
  const uint32_t at = data_bytes >> 3;
  const uint64_t bit = 0x80ull << (56u - 8u * (data_bytes & 7u));
#pragma unroll
  for (int j = 0; j < 8; ++j) b.w[j] = d[j] | (at == (uint32_t)j ? bit : 0ull);
  b.w[8] = at == 8u ? bit : 0ull;
#pragma unroll
  for (int j = 9; j < 15; ++j) b.w[j] = 0u;
  b.w[15] = (128ull + data_bytes) * 8u;
  return b;
}
// the midstates of an HMAC key of at most 128 bytes, given as its block (big-endian words, zero-padded): the states after the ipad and the opad block
struct hmac512_key { sha512_state inner, outer; };
ECS_DEV hmac512_key hmac512_key_from(const sha512_block& key) {
  sha512_block bi, bo;
#pragma unroll
  for (int j = 0; j < 16; ++j) { bi.w[j] = key.w[j] ^ 0x3636363636363636ull; bo.w[j] = key.w[j] ^ 0x5c5c5c5c5c5c5c5cull; }
  hmac512_key k;
  k.inner = sha512_iv(); sha512_compress(k.inner, bi);
  k.outer = sha512_iv(); sha512_compress(k.outer, bo);
  return k;
}
// the outer hash: H(opad block || inner digest)
ECS_DEV sha512_state hmac512_finish(const sha512_state& outer, const sha512_state& inner) {
  sha512_state o = outer;
  sha512_compress(o, sha512_tail_block64(inner, 192u));
  return o;
}

}  // namespace ecsimd_hip
