// fe381.cuh -- arithmetic modulo the BLS12-381 base field prime p (381 bits, dense), one element per lane.
//
// REPRESENTATION: twelve saturated 32-bit words (fe384.cuh's struct and word helpers), MONTGOMERY form with R = 2^384, and ALWAYS CANONICAL: every value
// inside the layer is a R mod p as an integer below p.  The three spare bits of 384 are NOT used for lazy additions: every function below takes operands
// below p and returns a result below p, so equality is a comparison of words, "is zero" is twelve ORs, and the exceptional cases of the group law (g1.cuh
// decides them on H = 0 and r = 0) need no normalisation first.  The cost is one conditional subtraction per addition; nobody has measured the lazy form.
//   THE DOOR: fe381_to_mont takes ANY 384-bit value v (2^384 < 10 p) and returns v R mod p, canonical -- the Montgomery product of v and R^2 mod p:
//   v (R^2 mod p) < R p, which is all the reduction asks (below).  So raw 48-byte records of any value are accepted as the residue they represent.
//   fe381_below_p is the wire format's own test (a coordinate >= p is malformed there, never reduced).
//
// PRODUCT: fe384.cuh's Comba columns (mul12x12: 144 multiply-adds; sqr12: 78).
// REDUCTION: word-serial Montgomery (REDC) over the 24-word product t, twelve passes: m = t[i] (-1/p mod 2^32), t += m p 2^(32 i) -- twelve multiply-adds
// a pass, 144 in all, each (uint64) m p[j] + t[i + j] + carry <= 2^64 - 1 -- with the carry out of a pass going to word i + 12 and one carry bit `top`
// travelling with it.  For t < R p the quotient t / R + (sum m_i 2^(32 i)) p / R is below 2 p < 2^382: `top` ends 0 and ONE conditional subtraction of p
// makes the result canonical.  -1/p mod 2^32 = 0xfffcfffd is no power of two, so the quotient digit costs a multiplication (P-384's is the raw word).
// A product is therefore 288 multiply-adds and a squaring 222 (tools/bls12_381_listing.py reports what the compiler makes of them).
//
// Inversion is a^(p - 2) and the square root a^((p + 1) / 4) (p = 3 mod 4), both by square-and-multiply over the bits of the PUBLIC exponent as loop
// constants.  Branches on data appear from g1.cuh upwards only; this layer selects by masks.
//
// Every function is __host__ __device__ (the column multiply-add is plain C++ on the host), so tests/cpp/bls12_381_host_check.cpp runs this very code on a CPU.
#pragma once
#include "fe384.cuh"

namespace ecsimd_hip {

using fe381 = fe384;                                                  // twelve words, w[0] the least significant

struct bls381_consts {
  static constexpr uint32_t P[12] = {0xffffaaabu, 0xb9feffffu, 0xb153ffffu, 0x1eabfffeu, 0xf6b0f624u, 0x6730d2a0u, 0xf38512bfu, 0x64774b84u, 0x434bacd7u, 0x4b1ba7b6u, 0x397fe69au, 0x1a0111eau};
  static constexpr uint32_t R1[12] = {0x0002fffdu, 0x76090000u, 0xc40c0002u, 0xebf4000bu, 0x53c758bau, 0x5f489857u, 0x70525745u, 0x77ce5853u, 0xa256ec6du, 0x5c071a97u, 0xfa80e493u, 0x15f65ec3u};   // R mod p: one
  static constexpr uint32_t R2[12] = {0x1c341746u, 0xf4df1f34u, 0x09d104f1u, 0x0a76e6a6u, 0x4c95b6d5u, 0x8de5476cu, 0x939d83c0u, 0x67eb88a9u, 0xb519952du, 0x9a793e85u, 0x92cae3aau, 0x11988fe5u};   // R^2 mod p
  static constexpr uint32_t B4[12] = {0x000cfff3u, 0xaa270000u, 0xfc34000au, 0x53cc0032u, 0x6b0a807fu, 0x478fe97au, 0xe6ba24d7u, 0xb1d37ebeu, 0xbf78ab2fu, 0x8ec9733bu, 0x3d83de7eu, 0x09d64551u};   // 4 R mod p: the curve's b
  static constexpr uint32_t P_MINUS_2[12] = {0xffffaaa9u, 0xb9feffffu, 0xb153ffffu, 0x1eabfffeu, 0xf6b0f624u, 0x6730d2a0u, 0xf38512bfu, 0x64774b84u, 0x434bacd7u, 0x4b1ba7b6u, 0x397fe69au, 0x1a0111eau};
  static constexpr uint32_t P_PLUS_1_DIV_4[12] = {0xffffeaabu, 0xee7fbfffu, 0xac54ffffu, 0x07aaffffu, 0x3dac3d89u, 0xd9cc34a8u, 0x3ce144afu, 0xd91dd2e1u, 0x90d2eb35u, 0x92c6e9edu, 0x8e5ff9a6u, 0x0680447au};
  static constexpr uint32_t HALF[12] = {0xffffd555u, 0xdcff7fffu, 0x58a9ffffu, 0x0f55ffffu, 0x7b587b12u, 0xb3986950u, 0x79c2895fu, 0xb23ba5c2u, 0x21a5d66bu, 0x258dd3dbu, 0x1cbff34du, 0x0d0088f5u};   // (p - 1) / 2
  static constexpr uint32_t NEG_INV32 = 0xfffcfffdu;                  // -1/p mod 2^32
};

ECS_HD fe381 fe381_zero() { return fe384_small(0u); }
ECS_HD fe381 fe381_one() { return fe384_const<bls381_consts::R1>(); }
ECS_HD bool fe381_is_zero(const fe381& a) { return fe384_is_zero(a) != 0u; }
ECS_HD bool fe381_equal(const fe381& a, const fe381& b) { return fe384_equal(a, b) != 0u; }
ECS_HD bool fe381_below_p(const fe381& a) { return w384_less(a, fe384_const<bls381_consts::P>()) != 0u; }   // any twelve words

// operands and results below p
ECS_HD fe381 fe381_add(const fe381& a, const fe381& b) { return mod384_add<bls381_consts::P>(a, b); }
ECS_HD fe381 fe381_sub(const fe381& a, const fe381& b) { return mod384_sub<bls381_consts::P>(a, b); }
ECS_HD fe381 fe381_neg(const fe381& a) { return mod384_sub<bls381_consts::P>(fe384_small(0u), a); }
ECS_HD fe381 fe381_dbl(const fe381& a) { return fe381_add(a, a); }

// t / R mod p for t < R p (see the head of the file); the result is below p
ECS_HD fe381 fe381_redc(const fe768& t) {
  uint32_t w[24];
#pragma unroll
  for (int i = 0; i < 24; ++i) w[i] = t.w[i];
  uint32_t top = 0;
#pragma unroll
  for (int i = 0; i < 12; ++i) {
    const uint32_t m = w[i] * bls381_consts::NEG_INV32;
    uint64_t acc = 0;
#pragma unroll
    for (int j = 0; j < 12; ++j) { acc += (uint64_t)m * bls381_consts::P[j] + w[i + j]; w[i + j] = (uint32_t)acc; acc >>= 32; }
    acc += (uint64_t)w[i + 12] + top;
    w[i + 12] = (uint32_t)acc;
    top = (uint32_t)(acc >> 32);
  }
  fe381 r;
#pragma unroll
  for (int i = 0; i < 12; ++i) r.w[i] = w[12 + i];
  return w384_cond_sub<bls381_consts::P>(r, 0u - top);               // top is 0 for t < R p; kept in the subtraction so that a wrong caller is not silently wrong twice
}
// a b / R: ONE operand may be any 384-bit value, the other is below p
ECS_HD fe381 fe381_mul(const fe381& a, const fe381& b) { return fe381_redc(mul12x12(a, b)); }
ECS_HD fe381 fe381_sqr(const fe381& a) { return fe381_redc(sqr12(a)); }
ECS_HD fe381 fe381_to_mont(const fe381& v) { return fe381_mul(v, fe384_const<bls381_consts::R2>()); }          // any 384-bit v
ECS_HD fe381 fe381_from_mont(const fe381& a) {                                                                  // the plain residue, below p
  fe768 t;
#pragma unroll
  for (int i = 0; i < 12; ++i) { t.w[i] = a.w[i]; t.w[12 + i] = 0u; }
  return fe381_redc(t);
}
// a^e for the public twelve-word exponent E, most significant bit first (0^e = 0 for e > 0)
template <const uint32_t (&E)[12]> ECS_HD fe381 fe381_pow(const fe381& a) {
  fe381 r = fe381_one();
#pragma unroll 1
  for (int w = 11; w >= 0; --w) {
    uint32_t e = 0;
#pragma unroll
    for (int q = 0; q < 12; ++q) e = w == q ? E[q] : e;               // w is a loop counter: uniform selects of literals
#pragma unroll 1
    for (int b = 31; b >= 0; --b) {
      r = fe381_sqr(r);
      if ((e >> b) & 1u) r = fe381_mul(r, a);                         // a bit of the exponent: public, the same on every lane
    }
  }
  return r;
}
ECS_HD fe381 fe381_invert(const fe381& a) { return fe381_pow<bls381_consts::P_MINUS_2>(a); }                    // 0 -> 0
// a square root of a, and whether a has one (p = 3 mod 4: a^((p + 1) / 4), checked by squaring)
ECS_HD fe381 fe381_sqrt(const fe381& a, bool& ok) {
  const fe381 s = fe381_pow<bls381_consts::P_PLUS_1_DIV_4>(a);
  ok = fe381_equal(fe381_sqr(s), a);
  return s;
}
// "lexicographically largest" of the serialisation: the plain residue y > (p - 1) / 2
ECS_HD bool fe381_lex_largest(const fe381& a) { return w384_less(fe384_const<bls381_consts::HALF>(), fe381_from_mont(a)) != 0u; }

}  // namespace ecsimd_hip
