// x25519.cuh -- the Montgomery curve v^2 = u^3 + 486662 u^2 + u over 2^255 - 19 (RFC 7748), x-only, on fe25519.cuh's field, and the two maps between it and
// the twisted Edwards curve of ed25519.cuh: u = (1 + y) / (1 - y) = (Z + Y) / (Z - Y).
//
//   * fe25519_mul_small   a * c for a 32-bit constant c: eight multiply-adds and the fold of a carry word.
//   * x25519_ladder       the x-coordinate of [k mod 2^255] u for SECRET k and ANY 256-bit representative u (a point of the curve, of its twist, or neither:
//                         the formulas ask nothing of u): 255 steps of RFC 7748 section 5's ladder, 5 M + 4 S + one product by a24 = 121665 + 8 additions each;
//                         the conditional swaps are XOR masks with the swap deferred into the next step (swap ^= k_t); the scalar's bits leave at the top of
//                         its words by shifting them, never by an index; one inversion and one canonical reduction at the end.  0 at infinity (0^(p - 2) = 0).
//   * x25519_base_ct      X25519(k, 9) for a CLAMPED secret k without the ladder: B = (.., 4/5) maps to u = 9 and has order L, so [k]9 is the image of
//                         [k mod L]B -- ed25519.cuh's comb, 64 mixed additions -- under the map above.  8 L > 2^255 > k, and k is a multiple of 8, so k is
//                         no multiple of L, [k mod L]B is not the identity and Z - Y is not zero.
//   * ed_to_mont          the u of an Ed25519 public key, PUBLIC data: strict decoding, the eight small-order encodings refused.
// No branch, address or lane mask here is made of a secret; everything is selected by masks.
#pragma once
#include "ed25519.cuh"
#include "sha512.cuh"

namespace ecsimd_hip {

constexpr uint32_t X25519_A24 = 121665u;                         // (486662 - 2) / 4

// a c as a representative, for any c < 2^32 / 38 (the ninth word of the product is below c, and 38 times it must fit the fold's first addition)
ECS_DEV fe fe25519_mul_small(const fe& a, uint32_t c) {
  fe r;
  uint64_t acc = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    acc += (uint64_t)a.w[i] * c;                                 // < 2^32 c + c: no overflow
    r.w[i] = (uint32_t)acc;
    acc >>= 32;
  }
  return fe25519_fold_carry(r, (uint32_t)acc);                   // the top word: below 2^17 for a24, times 38 below 2^23
}

// masked swap: m all ones -> (a, b) = (b, a)
ECS_DEV void fe25519_cswap(uint32_t m, fe& a, fe& b) {
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const uint32_t t = (a.w[i] ^ b.w[i]) & m;
    a.w[i] ^= t;
    b.w[i] ^= t;
  }
}
ECS_DEV void x25519_shl1(fe& v) {
#pragma unroll
  for (int j = 7; j > 0; --j) v.w[j] = __builtin_amdgcn_alignbit(v.w[j], v.w[j - 1], 31);
  v.w[0] <<= 1;
}

// the x-coordinate of [k mod 2^255] (the point whose x-coordinate is x1), canonical; 0 at infinity
ECS_DEV fe x25519_ladder(const fe& k, const fe& x1) {
  fe bits = k;
  x25519_shl1(bits);                                             // bit 255 leaves; bit 254 is now the top bit
  fe x2 = fe25519_small(1u), z2 = fe25519_small(0u), x3 = x1, z3 = fe25519_small(1u);
  uint32_t swap = 0;
#pragma unroll 1
  for (int t = 254; t >= 0; --t) {
    const uint32_t kt = 0u - (bits.w[7] >> 31);
    x25519_shl1(bits);
    swap ^= kt;
    fe25519_cswap(swap, x2, x3);
    fe25519_cswap(swap, z2, z3);
    swap = kt;
    const fe A = fe25519_add(x2, z2), B = fe25519_sub(x2, z2), AA = fe25519_sqr(A), BB = fe25519_sqr(B), E = fe25519_sub(AA, BB);
    const fe C = fe25519_add(x3, z3), D = fe25519_sub(x3, z3), DA = fe25519_mul(D, A), CB = fe25519_mul(C, B);
    x3 = fe25519_sqr(fe25519_add(DA, CB));
    z3 = fe25519_mul(x1, fe25519_sqr(fe25519_sub(DA, CB)));
    x2 = fe25519_mul(AA, BB);
    z2 = fe25519_mul(E, fe25519_add(AA, fe25519_mul_small(E, X25519_A24)));
  }
  fe25519_cswap(swap, x2, x3);
  fe25519_cswap(swap, z2, z3);
  return fe25519_canon(fe25519_mul(x2, fe25519_invert(z2)));
}

// RFC 7748 section 5's decodeScalar25519
ECS_DEV fe x25519_clamp(fe k) {
  k.w[0] &= 0xfffffff8u;
  k.w[7] = (k.w[7] & 0x7fffffffu) | 0x40000000u;
  return k;
}
// all ones where v is not all zero
ECS_DEV uint32_t x25519_nonzero_mask(const fe& v) {
  uint32_t d = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) d |= v.w[i];
  return (uint32_t)((int32_t)(d | (0u - d)) >> 31);
}

// (Z + Y) / (Z - Y), canonical: the u of the Edwards point p (0 for the identity, whose Z - Y is 0)
ECS_DEV fe ed_point_to_mont(const ed_point& p) {
  return fe25519_canon(fe25519_mul(fe25519_add(p.Z, p.Y), fe25519_invert(fe25519_sub(p.Z, p.Y))));
}
// X25519(k, 9) for a clamped k; M = L's gmod
ECS_DEV fe x25519_base_ct(const fe& clamped, const gmod& M) { return ed_point_to_mont(ed_base_ct(ed_sc_reduce256(clamped, M))); }

// all ones where enc is one of the eight encodings of the points of order 1, 2, 4 and 8 (k_ed25519.hip's list, held to the model by the tests)
ECS_DEV uint32_t x25519_bytes_equal_mask(const fe& a, const fe& b) {
  uint32_t d = 0;
#pragma unroll
  for (int q = 0; q < 8; ++q) d |= a.w[q] ^ b.w[q];
  return (uint32_t)((int32_t)((d | (0u - d)) ^ 0x80000000u) >> 31);
}
ECS_DEV uint32_t x25519_ed_small_order_mask(const fe& enc) {
  constexpr uint32_t S[3][8] = {
      {0xffffffecu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0x7fffffffu},      // y = p - 1: order 2
      {0x706a17c7u, 0x4fd84d3du, 0x760b3cbau, 0x0f67100du, 0xfa53202au, 0xc6cc392cu, 0x77fdc74eu, 0x7a03ac92u},      // order 8
      {0x8f95e826u, 0xb027b2c2u, 0x89f4c345u, 0xf098eff2u, 0x05acdfd5u, 0x3933c6d3u, 0x880238b1u, 0x05fc536du}};     // order 8
  fe y = enc;
  y.w[7] &= 0x7fffffffu;                                         // y = 0 and the two of order 8 with either sign, 1 and p - 1 as they are (x = 0)
  uint32_t hit = x25519_bytes_equal_mask(y, fe25519_small(0u)) | x25519_bytes_equal_mask(enc, fe25519_small(1u));
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    fe c;
#pragma unroll
    for (int q = 0; q < 8; ++q) c.w[q] = S[k][q];
    hit |= x25519_bytes_equal_mask(k == 0 ? enc : y, c);
  }
  return hit;
}
// u = (1 + y) / (1 - y) of an Ed25519 public key; all ones where it decodes by ed_decode's rules and is no small-order encoding, and u = 0 where not.
// PUBLIC data.  The sign of x is dropped: a key and its negative give the same u.
ECS_DEV uint32_t ed_to_mont(fe& u, const fe& enc) {
  ed_point p;
  const uint32_t ok = ed_decode(p, enc) & ~x25519_ed_small_order_mask(enc);
  u = fe25519_select(ok, ed_point_to_mont(p), fe25519_small(0u));
  return ok;
}

// the clamped low half of SHA-512(seed) for a 32-byte seed: ONE compression of a block of fixed shape (the seed, 0x80, zeros, the length 256 bits).
// seed and result are little-endian integers of the 32 bytes.
ECS_DEV fe x25519_scalar_of_seed(const fe& seed) {
  sha512_block m;
#pragma unroll
  for (int j = 0; j < 4; ++j) m.w[j] = sha512_join(__builtin_bswap32(seed.w[2 * j]), __builtin_bswap32(seed.w[2 * j + 1]));
  m.w[4] = 0x8000000000000000ull;
#pragma unroll
  for (int j = 5; j < 15; ++j) m.w[j] = 0u;
  m.w[15] = 256u;
  sha512_state s = sha512_iv();
  sha512_compress(s, m);
  fe r;
#pragma unroll
  for (int j = 0; j < 4; ++j) { r.w[2 * j] = __builtin_bswap32((uint32_t)(s.h[j] >> 32)); r.w[2 * j + 1] = __builtin_bswap32((uint32_t)s.h[j]); }
  return x25519_clamp(r);
}

}  // namespace ecsimd_hip
