// sm3.cuh -- SM3 (GB/T 32905-2016, ISO/IEC 10118-3) with one message per lane, and the two shapes the SM2 signature scheme puts on top of it:
// Z_A = SM3(ENTL || ID || a || b || x_G || y_G || x_A || y_A) and e = SM3(Z_A || M) with Z_A in registers.
//
// The compression function is written the way sha256.cuh's is: eight state words and a sixteen-word rolling schedule in registers, all 64 rounds unrolled
// so that every schedule index is a compile-time value (an array indexed by a loop variable would go to scratch memory) and the rotated round constants are
// literals.  Rotations are funnel shifts of a word with itself (v_alignbit_b32); FF and GG of rounds 16 - 63 are bit selects (the majority
// bfi(x ^ y, z, y) and the choice bfi(x, y, z): v_bfi_b32 forms, one three-input v_bitop3_b32 each on gfx950); in rounds 0 - 15 both are x ^ y ^ z.
// Round j needs W_j and W_(j+4): the slot of W_(j-12) takes W_(j+4) just before round j reads it.
//
// Words are big-endian throughout, as SM3 reads them: a 256-bit integer held as eight little-endian 32-bit words w[0..7] enters a block as w[7], ..., w[0],
// and a digest V0..V7 IS the integer with w[7 - j] = Vj -- no byte swap anywhere.
//
// Plain C++ only, and nothing here needs field.cuh: every function is __host__ __device__, so tests/cpp/sm2_host_check.cpp runs the very same text on the
// CPU against Python integers.  Public data throughout (messages, identities, public keys): the walkers branch on lengths.
#pragma once
#include <stddef.h>
#include <stdint.h>

#define SM3_FN __host__ __device__ __forceinline__

namespace ecsimd_hip {

struct sm3_state { uint32_t h[8]; };
struct sm3_block { uint32_t w[16]; };

SM3_FN uint32_t sm3_rotl(uint32_t x, int n) { return (n & 31) == 0 ? x : (x << (n & 31)) | (x >> (32 - (n & 31))); }      // n is a literal at every use
SM3_FN uint32_t sm3_bfi(uint32_t m, uint32_t a, uint32_t b) { return b ^ (m & (a ^ b)); }                                 // m ? a : b bit by bit
SM3_FN uint32_t sm3_p0(uint32_t x) { return x ^ sm3_rotl(x, 9) ^ sm3_rotl(x, 17); }
SM3_FN uint32_t sm3_p1(uint32_t x) { return x ^ sm3_rotl(x, 15) ^ sm3_rotl(x, 23); }

SM3_FN sm3_state sm3_iv() {
  sm3_state s;
  s.h[0] = 0x7380166fu; s.h[1] = 0x4914b2b9u; s.h[2] = 0x172442d7u; s.h[3] = 0xda8a0600u;
  s.h[4] = 0xa96f30bcu; s.h[5] = 0x163138aau; s.h[6] = 0xe38dee4du; s.h[7] = 0xb0fb0e4eu;
  return s;
}

// one block into the state; the block is taken by value (the schedule rolls over it)
SM3_FN void sm3_compress(sm3_state& s, sm3_block m) {
  uint32_t a = s.h[0], b = s.h[1], c = s.h[2], d = s.h[3], e = s.h[4], f = s.h[5], g = s.h[6], h = s.h[7];
#pragma unroll
  for (int j = 0; j < 64; ++j) {
    if (j >= 12) {                                            // W_(j+4) = P1(W_(j-12) ^ W_(j-5) ^ (W_(j+1) <<< 15)) ^ (W_(j-9) <<< 7) ^ W_(j-2)
      const uint32_t x = m.w[(j + 4) & 15] ^ m.w[(j - 5) & 15] ^ sm3_rotl(m.w[(j + 1) & 15], 15);
      m.w[(j + 4) & 15] = sm3_p1(x) ^ sm3_rotl(m.w[(j - 9) & 15], 7) ^ m.w[(j - 2) & 15];
    }
    const uint32_t w = m.w[j & 15], w1 = w ^ m.w[(j + 4) & 15];
    const uint32_t tj = sm3_rotl(j < 16 ? 0x79cc4519u : 0x7a879d8au, j & 31);
    const uint32_t a12 = sm3_rotl(a, 12);
    const uint32_t ss1 = sm3_rotl(a12 + e + tj, 7), ss2 = ss1 ^ a12;
    const uint32_t ff = j < 16 ? (a ^ b ^ c) : sm3_bfi(a ^ b, c, b);
    const uint32_t gg = j < 16 ? (e ^ f ^ g) : sm3_bfi(e, f, g);
    const uint32_t tt1 = ff + d + ss2 + w1, tt2 = gg + h + ss1 + w;
    d = c; c = sm3_rotl(b, 9); b = a; a = tt1;
    h = g; g = sm3_rotl(f, 19); f = e; e = sm3_p0(tt2);
  }
  s.h[0] ^= a; s.h[1] ^= b; s.h[2] ^= c; s.h[3] ^= d; s.h[4] ^= e; s.h[5] ^= f; s.h[6] ^= g; s.h[7] ^= h;
}

// ---- message bytes -> big-endian words.  ALIGNED: the address is a multiple of 4 (word loads), else byte loads.
// a where mask is all ones, b where it is zero -- as arithmetic on the address (sha256.cuh's msg_pick)
SM3_FN const uint8_t* sm3_pick(uint32_t mask, const uint8_t* a, const uint8_t* b) {
  const uintptr_t ia = reinterpret_cast<uintptr_t>(a), ib = reinterpret_cast<uintptr_t>(b);
  return reinterpret_cast<const uint8_t*>(ib + ((ia - ib) & (uintptr_t)(int64_t)(int32_t)mask));
}
SM3_FN uint32_t sm3_bswap(uint32_t v) { return __builtin_bswap32(v); }
template <bool ALIGNED> SM3_FN sm3_block sm3_load_block(const uint8_t* q) {
  sm3_block m;
  if constexpr (ALIGNED) {
    const uint32_t* p = reinterpret_cast<const uint32_t*>(q);
#pragma unroll
    for (int j = 0; j < 16; ++j) m.w[j] = sm3_bswap(p[j]);
  } else {
#pragma unroll
    for (int j = 0; j < 16; ++j) m.w[j] = ((uint32_t)q[4 * j] << 24) | ((uint32_t)q[4 * j + 1] << 16) | ((uint32_t)q[4 * j + 2] << 8) | (uint32_t)q[4 * j + 3];
  }
  return m;
}
// The last rem (0 .. 63) bytes at q, the byte `pad` (0x80: the padding's first byte; 0: nothing) right behind them, zeros.  No branch, and no byte at or
// behind q + rem is loaded (a row's tail need not be allocated): such a load is pointed at `spare` instead -- any readable, 4-byte aligned address -- and its
// value dropped, as in sha256.cuh's msg_tail_words_le.
template <bool ALIGNED> SM3_FN sm3_block sm3_load_tail(const uint8_t* q, uint32_t rem, const uint8_t* spare, uint32_t pad) {
  const uint32_t whole = rem >> 2, part = rem & 3u;            // words that are message bytes only; bytes of the one that is not
  uint32_t edge = pad << (24 - 8 * part);                      // that word: `part` message bytes, then the pad byte
  sm3_block m;
  if constexpr (ALIGNED) {
#pragma unroll
    for (uint32_t t = 0; t < 3; ++t) {
      const uint32_t have = 0u - (uint32_t)(t < part);
      const uint32_t b = *sm3_pick(have, q + 4 * whole + t, spare);
      edge |= (b & have) << (24 - 8 * t);
    }
#pragma unroll
    for (uint32_t k = 0; k < 16; ++k) {
      const uint32_t have = 0u - (uint32_t)(k < whole);
      m.w[k] = sm3_bswap(*reinterpret_cast<const uint32_t*>(sm3_pick(have, q + 4 * k, spare))) & have;
    }
  } else {
#pragma unroll
    for (uint32_t k = 0; k < 16; ++k) {
      uint32_t v = 0;
#pragma unroll
      for (uint32_t t = 0; t < 4; ++t) {
        const uint32_t have = 0u - (uint32_t)(4 * k + t < rem);
        const uint32_t b = *sm3_pick(have, q + 4 * k + t, spare);
        v |= (b & have) << (24 - 8 * t);
      }
      m.w[k] = v;                                              // (the edge word holds its message bytes already: the pad byte joins them below)
    }
  }
#pragma unroll
  for (uint32_t k = 0; k < 16; ++k) m.w[k] |= edge & (0u - (uint32_t)(k == whole));
  return m;
}

// SM3 of the len bytes at p, a length of the lane's own (the shape of sha256_absorb_message_lens): whole blocks go through THE loop of this function,
// len / 64 trips; the tail block comes from sm3_load_tail, and where fewer than 9 bytes are free behind the message a block of zeros follows it.
template <bool ALIGNED> SM3_FN void sm3_absorb_message(sm3_state& s, const uint8_t* p, uint32_t len, const uint8_t* spare) {
  const uint32_t full = len >> 6, rem = len & 63u;
#pragma unroll 1
  for (uint32_t b = 0; b < full; ++b) {
    sm3_compress(s, sm3_load_block<ALIGNED>(p));
    p += 64;
  }
  sm3_block m = sm3_load_tail<ALIGNED>(p, rem, spare, 0x80u);
  const uint32_t tails = rem >= 56u ? 2u : 1u;
#pragma unroll 1
  for (uint32_t t = 0; t < tails; ++t) {
    if (t + 1 == tails) { m.w[14] = len >> 29; m.w[15] = len << 3; }
    sm3_compress(s, m);
#pragma unroll
    for (int j = 0; j < 16; ++j) m.w[j] = 0u;
  }
}

// The rest of a hash whose first 32 bytes are the eight words z (SM2's e = SM3(Z_A || M)): every block is half carried over, half loaded.  len < 2^31.
// The tail block holds 32 + rem + 1 bytes: up to rem = 23 the bit length fits behind them, from 24 on a second block takes it.
template <bool ALIGNED> SM3_FN void sm3_absorb_after32(sm3_state& s, const uint32_t (&z)[8], const uint8_t* p, uint32_t len, const uint8_t* spare) {
  const uint32_t full = len >> 6, rem = len & 63u;
  sm3_block m;
#pragma unroll
  for (int j = 0; j < 8; ++j) m.w[j] = z[j];
#pragma unroll 1
  for (uint32_t b = 0; b < full; ++b) {
    const sm3_block x = sm3_load_block<ALIGNED>(p);
#pragma unroll
    for (int j = 0; j < 8; ++j) m.w[8 + j] = x.w[j];
    sm3_compress(s, m);
#pragma unroll
    for (int j = 0; j < 8; ++j) m.w[j] = x.w[8 + j];
    p += 64;
  }
  const sm3_block x = sm3_load_tail<ALIGNED>(p, rem, spare, 0x80u);
#pragma unroll
  for (int j = 0; j < 8; ++j) m.w[8 + j] = x.w[j];
  const uint32_t tails = rem >= 24u ? 2u : 1u, total = len + 32u;
#pragma unroll 1
  for (uint32_t t = 0; t < tails; ++t) {
    if (t + 1 == tails) { m.w[14] = total >> 29; m.w[15] = total << 3; }
    sm3_compress(s, m);
#pragma unroll
    for (int j = 0; j < 8; ++j) { m.w[j] = x.w[8 + j]; m.w[8 + j] = 0u; }
  }
}

// ---- a byte stream whose pieces do not lie on the word grid (Z_A: two bytes of ENTL, then ID, then 192 bytes of integers).  The open block st.w holds
// `fill` bytes (0 .. 63) and zeros behind them.  fill is the SAME on every lane of a launch -- it comes from id_bytes, a kernel argument -- so the shifts
// below are uniform branches over compile-time register indices: a byte shift by fill mod 4 (funnel shifts), then a barrel shifter by fill / 4 words.
struct sm3_stream { sm3_state s; uint32_t w[16]; };
template <int B> SM3_FN void sm3_words_up(uint32_t (&z)[32]) {
#pragma unroll
  for (int j = 31; j >= B; --j) z[j] = z[j - B];
#pragma unroll
  for (int j = 0; j < B; ++j) z[j] = 0u;
}
// The first `count` (1 .. 64) bytes of x behind the stream's; the words of x behind them must be zero.  A block that fills up is compressed.  The caller
// keeps the count: fill' = (fill + count) mod 64.
SM3_FN void sm3_push(sm3_stream& st, uint32_t fill, const sm3_block& x, uint32_t count) {
  const uint32_t sh = 8u * (fill & 3u), q = fill >> 2;
  uint32_t z[32];
  z[0] = x.w[0] >> sh;
#pragma unroll
  for (int j = 1; j < 16; ++j) z[j] = (uint32_t)(((((uint64_t)x.w[j - 1]) << 32) | x.w[j]) >> sh);
  z[16] = (uint32_t)((((uint64_t)x.w[15]) << 32) >> sh);
#pragma unroll
  for (int j = 17; j < 32; ++j) z[j] = 0u;
  if (q & 8u) sm3_words_up<8>(z);
  if (q & 4u) sm3_words_up<4>(z);
  if (q & 2u) sm3_words_up<2>(z);
  if (q & 1u) sm3_words_up<1>(z);
#pragma unroll
  for (int j = 0; j < 16; ++j) st.w[j] |= z[j];
  if (fill + count >= 64u) {
    sm3_block m;
#pragma unroll
    for (int j = 0; j < 16; ++j) { m.w[j] = st.w[j]; st.w[j] = z[16 + j]; }
    sm3_compress(st.s, m);
  }
}
// the padding and the bit length behind a stream of total_bytes bytes, fill = total_bytes mod 64
SM3_FN void sm3_finish(sm3_stream& st, uint32_t fill, uint32_t total_bytes) {
  sm3_block pad;
#pragma unroll
  for (int j = 0; j < 16; ++j) pad.w[j] = j == 0 ? 0x80000000u : 0u;
  sm3_push(st, fill, pad, 1u);
  sm3_block m;
#pragma unroll
  for (int j = 0; j < 16; ++j) m.w[j] = st.w[j];
  if (((fill + 1u) & 63u) > 56u) {                            // (0: the block was full and has just been compressed; the length opens the next one)
    sm3_compress(st.s, m);
#pragma unroll
    for (int j = 0; j < 16; ++j) m.w[j] = 0u;
  }
  m.w[14] = total_bytes >> 29; m.w[15] = total_bytes << 3;
  sm3_compress(st.s, m);
}

// Z_A (GB/T 32918.2 5.5): SM3(ENTL || ID || t), ENTL = the bit length of ID as two big-endian bytes, t = a, b, x_G, y_G, x_A, y_A as 48 big-endian words.
// id_bytes <= 8191 (ENTL has 16 bits) and is the same on every lane; the ID bytes are the lane's own (any alignment: byte loads).  `spare`: sm3_load_tail's.
SM3_FN sm3_state sm3_za(const uint8_t* id, uint32_t id_bytes, const uint8_t* spare, const uint32_t (&t)[48]) {
  sm3_stream st;
  st.s = sm3_iv();
#pragma unroll
  for (int j = 0; j < 16; ++j) st.w[j] = 0u;
  st.w[0] = (id_bytes << 3) << 16;
  const uint32_t full = id_bytes >> 6, rem = id_bytes & 63u;
#pragma unroll 1
  for (uint32_t b = 0; b < full; ++b) {
    sm3_push(st, 2u, sm3_load_block<false>(id), 64u);
    id += 64;
  }
  if (rem) sm3_push(st, 2u, sm3_load_tail<false>(id, rem, spare, 0u), rem);
  const uint32_t fill = (2u + rem) & 63u;
#pragma unroll 1
  for (int part = 0; part < 3; ++part) {
    sm3_block x;
#pragma unroll
    for (int j = 0; j < 16; ++j) x.w[j] = part == 0 ? t[j] : part == 1 ? t[16 + j] : t[32 + j];
    sm3_push(st, fill, x, 64u);
  }
  sm3_finish(st, fill, 2u + id_bytes + 192u);
  return st.s;
}

// ---- the integer arithmetic of the PUBLIC half of the scheme (verification; GB/T 32918.2 7.1), on eight little-endian words, plain C++: what
// k_sm2_verify_scalars and k_sm2_accept compute, and what the host check feeds edge values through.
struct sm2_int { uint32_t w[8]; };
SM3_FN uint32_t sm2_add(sm2_int& r, const sm2_int& a, const sm2_int& b) {          // the carry out
  uint64_t c = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) { c += (uint64_t)a.w[j] + b.w[j]; r.w[j] = (uint32_t)c; c >>= 32; }
  return (uint32_t)c;
}
SM3_FN uint32_t sm2_sub(sm2_int& r, const sm2_int& a, const sm2_int& b) {          // the borrow out
  uint64_t c = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) { const uint64_t d = (uint64_t)a.w[j] - b.w[j] - c; r.w[j] = (uint32_t)d; c = (d >> 32) & 1u; }
  return (uint32_t)c;
}
SM3_FN uint32_t sm2_nonzero(const sm2_int& a) {
  uint32_t d = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) d |= a.w[j];
  return d != 0u ? 1u : 0u;
}
// a + carry 2^256 < 2n  ->  that value mod n
SM3_FN sm2_int sm2_reduce_once(const sm2_int& a, uint32_t carry, const sm2_int& n) {
  sm2_int d;
  const uint32_t below = sm2_sub(d, a, n);
  const uint32_t take = (carry | (below ^ 1u)) ? 0xffffffffu : 0u;
  sm2_int r;
#pragma unroll
  for (int j = 0; j < 8; ++j) r.w[j] = (d.w[j] & take) | (a.w[j] & ~take);
  return r;
}
SM3_FN uint32_t sm2_in_range(const sm2_int& v, const sm2_int& n) { sm2_int d; return sm2_nonzero(v) & sm2_sub(d, v, n); }          // 1 <= v < n
// valid = 1 <= r < n and 1 <= s < n and t != 0, t = (r + s) mod n; u1 = s, u2 = t, zeros where not valid
SM3_FN uint32_t sm2_verify_scalars(const sm2_int& r, const sm2_int& s, const sm2_int& n, sm2_int& u1, sm2_int& u2) {
  sm2_int sum;
  const uint32_t carry = sm2_add(sum, r, s);
  const sm2_int t = sm2_reduce_once(sum, carry, n);           // r, s < n where it counts
  const uint32_t valid = sm2_in_range(r, n) & sm2_in_range(s, n) & sm2_nonzero(t);
  const uint32_t keep = 0u - valid;
#pragma unroll
  for (int j = 0; j < 8; ++j) { u1.w[j] = s.w[j] & keep; u2.w[j] = t.w[j] & keep; }
  return valid;
}
// (e mod n + x mod n) mod n == r, for ANY 256-bit e and x (2^256 < 2n on a curve with the ECDSA capability: one conditional subtraction reduces each)
SM3_FN uint32_t sm2_accept(const sm2_int& e, const sm2_int& x, const sm2_int& r, const sm2_int& n) {
  const sm2_int em = sm2_reduce_once(e, 0u, n), xm = sm2_reduce_once(x, 0u, n);
  sm2_int sum;
  const uint32_t carry = sm2_add(sum, em, xm);
  const sm2_int big_r = sm2_reduce_once(sum, carry, n);
  uint32_t d = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) d |= big_r.w[j] ^ r.w[j];
  return d == 0u ? 1u : 0u;
}

}  // namespace ecsimd_hip
