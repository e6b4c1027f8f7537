// fe25519.cuh -- arithmetic modulo p = 2^255 - 19, one element per lane.
//
// Representation: field.cuh's `fe`, eight saturated 32-bit words, holding ANY representative in [0, 2^256) -- 2^256 = 2 p + 38, so every residue has two of
// them and the residues below 38 three.  Every function takes any representative and returns one; only fe25519_canon returns THE residue in [0, p), and the
// wire format and every comparison go through it.  The load rule for raw 256-bit inputs follows: all 2^256 values are accepted as they are (a value >= p is
// the residue it is congruent to).
//
// The product and the squaring are field.cuh's Comba columns (mul8x8, sqr8: 512 bits), folded by 2^256 = 38: lo + 38 hi is below 39 * 2^256, its ninth word
// (at most 38) folds once more, and the carry of that addition (the value then wraps to below 38 * 39) takes one last + 38 that cannot carry.  Addition and
// subtraction fold their carry / borrow the same way.  Plain C++ on top of the trusted columns; no branch, everything by masks, so the secret kernels of
// k_ed25519.hip use it as it is.  Nobody has measured this against reduced-radix limbs here.
#pragma once
#include "field.cuh"
#include "ed25519_base.inc"

namespace ecsimd_hip {

struct ed25519_consts {
  static constexpr uint32_t D[8] = ED25519_D_WORDS;            // -121665 / 121666
  static constexpr uint32_t D2[8] = ED25519_2D_WORDS;          // 2 d
  static constexpr uint32_t SQRTM1[8] = ED25519_SQRTM1_WORDS;  // 2^((p - 1) / 4)
  static constexpr uint32_t L[8] = ED25519_L_WORDS;            // the group order
};
template <const uint32_t (&ARR)[8]> ECS_DEV fe fe25519_const() {
  fe r;
#pragma unroll
  for (int i = 0; i < 8; ++i) r.w[i] = ARR[i];
  return r;
}
ECS_DEV fe fe25519_small(uint32_t v) {
  fe r;
  r.w[0] = v;
#pragma unroll
  for (int i = 1; i < 8; ++i) r.w[i] = 0u;
  return r;
}

// r + 38 * c for the carry word c <= 38 of a sum or a fold, and the + 38 of the wrap behind it
ECS_DEV fe fe25519_fold_carry(const fe& r, uint32_t c) {
  fe o;
  uint64_t acc = (uint64_t)r.w[0] + (uint64_t)c * 38u;
  o.w[0] = (uint32_t)acc;
#pragma unroll
  for (int i = 1; i < 8; ++i) { acc = (acc >> 32) + r.w[i]; o.w[i] = (uint32_t)acc; }
  const uint32_t again = (uint32_t)(acc >> 32) * 38u;           // 0 or 38: the value wrapped to below 38 * 39, this cannot carry out
  acc = (uint64_t)o.w[0] + again;
  o.w[0] = (uint32_t)acc;
#pragma unroll
  for (int i = 1; i < 8; ++i) { acc = (acc >> 32) + o.w[i]; o.w[i] = (uint32_t)acc; }
  return o;
}
// the 512-bit t modulo p, as a representative
ECS_DEV fe fe25519_fold(const fe2& t) {
  fe r;
  uint64_t acc = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    acc += (uint64_t)t.w[i] + (uint64_t)t.w[8 + i] * 38u;      // < 2^32 + 38 (2^32 - 1) + 38: no overflow
    r.w[i] = (uint32_t)acc;
    acc >>= 32;
  }
  return fe25519_fold_carry(r, (uint32_t)acc);
}
ECS_DEV fe fe25519_mul(const fe& a, const fe& b) { return fe25519_fold(mul8x8(a, b)); }
ECS_DEV fe fe25519_sqr(const fe& a) { return fe25519_fold(sqr8(a)); }
ECS_DEV fe fe25519_add(const fe& a, const fe& b) {
  fe s = a;
  const uint32_t c = add8(s, b);
  return fe25519_fold_carry(s, c);
}
// a - b: a borrow is - 2^256 = - 38 too much; taking 38 off may borrow once more (then the value is at least 2^256 - 76 and the second 38 comes off cleanly)
ECS_DEV fe fe25519_sub(const fe& a, const fe& b) {
  fe d = a;
  uint32_t m = sub8(d, b);
  m = sub8(d, fe25519_small(38u & m));
  (void)sub8(d, fe25519_small(38u & m));
  return d;
}
ECS_DEV fe fe25519_neg(const fe& a) { return fe25519_sub(fe25519_small(0u), a); }
// m (all ones / all zeros) ? a : b, by masks
ECS_DEV fe fe25519_select(uint32_t m, const fe& a, const fe& b) {
  fe r;
#pragma unroll
  for (int i = 0; i < 8; ++i) r.w[i] = (a.w[i] & m) | (b.w[i] & ~m);
  return r;
}
// THE residue in [0, p)
ECS_DEV fe fe25519_canon(const fe& a) {
  fe r = a;
#pragma unroll
  for (int pass = 0; pass < 2; ++pass) {                         // bit 255 is worth 19: twice, the second time the rest is below 38
    uint64_t acc = (uint64_t)r.w[0] + 19u * (r.w[7] >> 31);
    r.w[7] &= 0x7fffffffu;
    r.w[0] = (uint32_t)acc;
#pragma unroll
    for (int i = 1; i < 8; ++i) { acc = (acc >> 32) + r.w[i]; r.w[i] = (uint32_t)acc; }
  }
  fe t;                                                          // r < 2^255; r >= p  <=>  r + 19 reaches bit 255
  uint64_t acc = (uint64_t)r.w[0] + 19u;
  t.w[0] = (uint32_t)acc;
#pragma unroll
  for (int i = 1; i < 8; ++i) { acc = (acc >> 32) + r.w[i]; t.w[i] = (uint32_t)acc; }
  const uint32_t ge = 0u - (t.w[7] >> 31);
  t.w[7] &= 0x7fffffffu;
  return fe25519_select(ge, t, r);
}
// all ones where a = 0 (mod p)
ECS_DEV uint32_t fe25519_zero_mask(const fe& a) {
  const fe c = fe25519_canon(a);
  uint32_t d = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) d |= c.w[i];
  return (uint32_t)((int32_t)((d | (0u - d)) ^ 0x80000000u) >> 31);
}
ECS_DEV uint32_t fe25519_eq_mask(const fe& a, const fe& b) { return fe25519_zero_mask(fe25519_sub(a, b)); }
// a^(2^n), n >= 1, a loop left standing
ECS_DEV fe fe25519_sqrn(fe a, int n) {
#pragma unroll 1
  for (int i = 0; i < n; ++i) a = fe25519_sqr(a);
  return a;
}
// z^(2^250 - 1) and z^11, the common trunk of the two chains below
ECS_DEV fe fe25519_pow250(const fe& z, fe& z11) {
  const fe z2 = fe25519_sqr(z);
  const fe z9 = fe25519_mul(fe25519_sqrn(z2, 2), z);
  z11 = fe25519_mul(z9, z2);
  const fe z5_0 = fe25519_mul(fe25519_sqr(z11), z9);             // 2^5 - 1
  const fe z10_0 = fe25519_mul(fe25519_sqrn(z5_0, 5), z5_0);
  const fe z20_0 = fe25519_mul(fe25519_sqrn(z10_0, 10), z10_0);
  const fe z40_0 = fe25519_mul(fe25519_sqrn(z20_0, 20), z20_0);
  const fe z50_0 = fe25519_mul(fe25519_sqrn(z40_0, 10), z10_0);
  const fe z100_0 = fe25519_mul(fe25519_sqrn(z50_0, 50), z50_0);
  const fe z200_0 = fe25519_mul(fe25519_sqrn(z100_0, 100), z100_0);
  return fe25519_mul(fe25519_sqrn(z200_0, 50), z50_0);
}
// z^(p - 2) = z^(2^255 - 21): 254 squarings, 11 products; 0 -> 0
ECS_DEV fe fe25519_invert(const fe& z) {
  fe z11;
  const fe t = fe25519_pow250(z, z11);
  return fe25519_mul(fe25519_sqrn(t, 5), z11);
}
// z^((p - 5) / 8) = z^(2^252 - 3)
ECS_DEV fe fe25519_pow22523(const fe& z) {
  fe z11;
  const fe t = fe25519_pow250(z, z11);
  return fe25519_mul(fe25519_sqrn(t, 2), z);
}
// x = sqrt(u / v) for p = 5 mod 8: u v^3 (u v^7)^((p - 5) / 8), times sqrt(-1) where v x^2 = -u; returns all ones where a root exists (u = 0: x = 0, ones)
ECS_DEV uint32_t fe25519_sqrt_ratio(fe& x, const fe& u, const fe& v) {
  const fe v3 = fe25519_mul(fe25519_sqr(v), v);
  const fe v7 = fe25519_mul(fe25519_sqr(v3), v);
  x = fe25519_mul(fe25519_mul(u, v3), fe25519_pow22523(fe25519_mul(u, v7)));
  const fe vxx = fe25519_mul(v, fe25519_sqr(x));
  const uint32_t plain = fe25519_eq_mask(vxx, u), flipped = fe25519_zero_mask(fe25519_add(vxx, u));
  x = fe25519_select(flipped & ~plain, fe25519_mul(x, fe25519_const<ed25519_consts::SQRTM1>()), x);
  return plain | flipped;
}

}  // namespace ecsimd_hip
