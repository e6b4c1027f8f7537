// p384.cuh -- the group of NIST P-384 on fe384.cuh: y^2 = x^3 - 3 x + b over p, prime order n, cofactor 1.
//
// Points are homogeneous projective (X : Y : Z), the identity (0 : 1 : 0), under the COMPLETE formulas for a = -3 of Renes, Costello and Batina, "Complete
// addition formulas for prime order elliptic curves" (2016): Algorithm 4 (p384_add), Algorithm 5 (p384_add_mixed, the second operand affine and not the
// identity) and Algorithm 6 (p384_dbl).  One law for every input pair -- P + P, P + (-P), the identity on either side: there is no exceptional case to
// meet and none is tested for.  Algorithms 4 and 5 differ in how they form six products and sums and share everything behind them (p384_add_tail).
//
// Scalars go through SIGNED 4-bit digits: k + 0x88...8 (96 nibbles of 8) cut into nibbles n_i gives k = sum (n_i - 8) 16^i + c 16^96 with digits in
// [-8, 7] and c = the carry out of the addition, 0 or 1 (p384_digits).  The top nibble is read and the value shifted by four bits per window: no index is
// made of a digit.
//   * p384_base_ct   k G, SECRET k: a comb over P384_BASE, 25 rows of 1 .. 8 times 65536^j G, affine.  Digit 4 j + r goes with row j in pass r: passes
//     r = 3, 2, 1, 0 of 24 mixed additions each, four doublings between two passes, and one last addition for c from row 24 -- 97 mixed additions and 12
//     doublings.  Every entry of a row is read (the row's address is the loop counter's) and chosen and negated by masks.
//     Geometry: one row per digit (97 rows, no doubling) is the fastest and a 250 KB table in the source; every fourth row costs 12 doublings of 11 products
//     on top of 97 additions of 13 -- 10 % -- for a quarter of it (63 KB), and every eighth would cost 28.  Wider digits do not pay: all entries of a row are
//     read whatever the digit, so 5-bit digits take 77 additions for 16 entries per row.
//   * p384_var_ct    k P, SECRET k: 96 windows of four doublings and one complete addition of +-(0 .. 8) P from the lane's own table of 1 .. 8 P (in
//     memory, word-major: entry e's word w of lane i at table[(e * 36 + w) * lanes + i], so a wave reads consecutive words).  Every entry is read in every
//     window at an address that does not depend on the window, and chosen and negated by masks; digit 0 adds the identity, which the complete law takes.
//   * p384_double_mult  u1 G + u2 Q for verification (public data, the same masked code): one Straus loop, G's multiples from row 0 of P384_BASE, Q's
//     from the lane's table.
#pragma once
#include "fe384.cuh"

namespace ecsimd_hip {

__device__ const uint32_t P384_BASE[P384_BASE_WINDOWS * P384_BASE_ENTRIES * 24] = {P384_BASE_TABLE};

struct p384_point { fe384 X, Y, Z; };
struct p384_affine { fe384 x, y; };
constexpr int P384_TABLE_WORDS = 8 * 36;           // per lane: 1 .. 8 P, projective

ECS_HD p384_point p384_identity() { return {fe384_small(0u), fe384_small(1u), fe384_small(0u)}; }
ECS_HD p384_point p384_from_affine(const p384_affine& a) { return {a.x, a.y, fe384_small(1u)}; }
ECS_HD p384_point p384_select(uint32_t mask, const p384_point& a, const p384_point& b) {
  return {fe384_select(mask, a.X, b.X), fe384_select(mask, a.Y, b.Y), fe384_select(mask, a.Z, b.Z)};
}
ECS_HD uint32_t p384_is_identity(const p384_point& p) { return fe384_is_zero(p.Z); }

// Algorithm 4 from step 19 on.  t0 = X1 X2, t1 = Y1 Y2, t2 = Z1 Z2, t3 = X1 Y2 + X2 Y1, t4 = Y1 Z2 + Y2 Z1, y3 = X1 Z2 + X2 Z1.
ECS_HD p384_point p384_add_tail(fe384 t0, fe384 t1, fe384 t2, const fe384& t3, const fe384& t4, fe384 y3) {
  const fe384 b = fe384_const<p384_consts::B>();
  fe384 x3, z3;
  z3 = fe384_mul(b, t2); x3 = fe384_sub(y3, z3); z3 = fe384_dbl(x3);
  x3 = fe384_add(x3, z3); z3 = fe384_sub(t1, x3); x3 = fe384_add(t1, x3);
  y3 = fe384_mul(b, y3); t1 = fe384_dbl(t2); t2 = fe384_add(t1, t2);
  y3 = fe384_sub(y3, t2); y3 = fe384_sub(y3, t0); t1 = fe384_dbl(y3);
  y3 = fe384_add(t1, y3); t1 = fe384_dbl(t0); t0 = fe384_add(t1, t0);
  t0 = fe384_sub(t0, t2); t1 = fe384_mul(t4, y3); t2 = fe384_mul(t0, y3);
  y3 = fe384_mul(x3, z3); y3 = fe384_add(y3, t2); x3 = fe384_mul(t3, x3);
  x3 = fe384_sub(x3, t1); z3 = fe384_mul(t4, z3); t1 = fe384_mul(t3, t0);
  z3 = fe384_add(z3, t1);
  return {x3, y3, z3};
}
ECS_HD p384_point p384_add(const p384_point& p, const p384_point& q) {
  const fe384 t0 = fe384_mul(p.X, q.X), t1 = fe384_mul(p.Y, q.Y), t2 = fe384_mul(p.Z, q.Z);
  fe384 t3 = fe384_mul(fe384_add(p.X, p.Y), fe384_add(q.X, q.Y));
  t3 = fe384_sub(t3, fe384_add(t0, t1));
  fe384 t4 = fe384_mul(fe384_add(p.Y, p.Z), fe384_add(q.Y, q.Z));
  t4 = fe384_sub(t4, fe384_add(t1, t2));
  fe384 y3 = fe384_mul(fe384_add(p.X, p.Z), fe384_add(q.X, q.Z));
  y3 = fe384_sub(y3, fe384_add(t0, t2));
  return p384_add_tail(t0, t1, t2, t3, t4, y3);
}
ECS_HD p384_point p384_add_mixed(const p384_point& p, const p384_affine& q) {
  const fe384 t0 = fe384_mul(p.X, q.x), t1 = fe384_mul(p.Y, q.y);
  fe384 t3 = fe384_mul(fe384_add(q.x, q.y), fe384_add(p.X, p.Y));
  t3 = fe384_sub(t3, fe384_add(t0, t1));
  const fe384 t4 = fe384_add(fe384_mul(q.y, p.Z), p.Y);
  const fe384 y3 = fe384_add(fe384_mul(q.x, p.Z), p.X);
  return p384_add_tail(t0, t1, p.Z, t3, t4, y3);
}
ECS_HD p384_point p384_dbl(const p384_point& p) {
  const fe384 b = fe384_const<p384_consts::B>();
  fe384 t0 = fe384_sqr(p.X), t2 = fe384_sqr(p.Z), t3, x3, y3, z3;
  const fe384 t1 = fe384_sqr(p.Y);
  t3 = fe384_dbl(fe384_mul(p.X, p.Y)); z3 = fe384_dbl(fe384_mul(p.X, p.Z));
  y3 = fe384_sub(fe384_mul(b, t2), z3); x3 = fe384_dbl(y3); y3 = fe384_add(x3, y3);
  x3 = fe384_sub(t1, y3); y3 = fe384_add(t1, y3); y3 = fe384_mul(x3, y3);
  x3 = fe384_mul(x3, t3); t3 = fe384_dbl(t2); t2 = fe384_add(t2, t3);
  z3 = fe384_sub(fe384_sub(fe384_mul(b, z3), t2), t0); t3 = fe384_dbl(z3); z3 = fe384_add(z3, t3);
  t3 = fe384_dbl(t0); t0 = fe384_sub(fe384_add(t3, t0), t2); t0 = fe384_mul(t0, z3);
  y3 = fe384_add(y3, t0); t0 = fe384_dbl(fe384_mul(p.Y, p.Z)); z3 = fe384_mul(t0, z3);
  x3 = fe384_sub(x3, z3); z3 = fe384_mul(t0, t1); z3 = fe384_dbl(fe384_dbl(z3));
  return {x3, y3, z3};
}

// (x, y) of a point, (0, 0) for the identity: one inversion
ECS_HD p384_affine p384_to_affine(const p384_point& p) {
  const fe384 zi = fe384_invert(p.Z);
  return {fe384_mul(p.X, zi), fe384_mul(p.Y, zi)};
}
// mask: x, y < p as integers and y^2 = x^3 - 3 x + b.  The cofactor is 1: that is full validation.  (0, 0) is not on the curve (b != 0).
ECS_HD uint32_t p384_valid(const p384_affine& a) {
  const fe384 p = fe384_const<p384_consts::P>();
  const uint32_t in_range = w384_less(a.x, p) & w384_less(a.y, p);
  const fe384 x = fe384_canon(a.x), y = fe384_canon(a.y);
  fe384 rhs = fe384_mul(fe384_sqr(x), x);
  rhs = fe384_sub(rhs, fe384_add(fe384_dbl(x), x));
  rhs = fe384_add(rhs, fe384_const<p384_consts::B>());
  return in_range & fe384_equal(fe384_sqr(y), rhs);
}

// ---- 48 big-endian bytes <-> twelve little-endian words; aligned: the address is a multiple of 4
ECS_DEV fe384 p384_load48(const uint8_t* __restrict__ p, uint32_t aligned) {
  fe384 r;
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
ECS_DEV void p384_store48(uint8_t* __restrict__ p, const fe384& v, uint32_t aligned) {
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

// ---- signed digits.  d = k + 0x88...8 and its carry c; the windows read d's top nibble and shift.
struct p384_digits { fe384 d; uint32_t c; };
ECS_HD p384_digits p384_recode(const fe384& k) {
  fe384 eights;
#pragma unroll
  for (int i = 0; i < 12; ++i) eights.w[i] = 0x88888888u;
  p384_digits r;
  r.c = w384_add(r.d, k, eights);
  return r;
}
ECS_HD uint32_t p384_top_nibble(fe384& d) {                                     // the nibble, and d <<= 4
  const uint32_t nib = d.w[11] >> 28;
#pragma unroll
  for (int i = 11; i > 0; --i) d.w[i] = (d.w[i] << 4) | (d.w[i - 1] >> 28);
  d.w[0] <<= 4;
  return nib;
}
ECS_HD uint32_t p384_low_nibble(fe384& d) {                                     // the nibble, and d >>= 4
  const uint32_t nib = d.w[0] & 15u;
#pragma unroll
  for (int i = 0; i < 11; ++i) d.w[i] = (d.w[i] >> 4) | (d.w[i + 1] << 28);
  d.w[11] >>= 4;
  return nib;
}
// a nibble n stands for the digit n - 8: its magnitude (0 .. 8) and the mask of a negative digit
ECS_HD uint32_t p384_digit_mag(uint32_t nib, uint32_t& neg) {
  neg = 0u - ((nib >> 3) ^ 1u);
  const uint32_t v = nib - 8u;
  return (v ^ neg) - neg;
}
ECS_HD uint32_t p384_eq_mask(uint32_t a, uint32_t b) { return ~mask384_nonzero(a ^ b); }

// entry `mag` (1 .. 8; anything else: (0, 0)) of the row at t, every entry read
ECS_HD p384_affine p384_row_select(const uint32_t* __restrict__ t, uint32_t mag) {
  p384_affine r = {fe384_small(0u), fe384_small(0u)};
#pragma unroll 1                                                                 // one entry in flight: 24 words loaded, 24 kept
  for (int e = 0; e < P384_BASE_ENTRIES; ++e) {
    const uint32_t m = p384_eq_mask(mag, (uint32_t)e + 1u);
#pragma unroll
    for (int q = 0; q < 12; ++q) { r.x.w[q] |= t[24 * e + q] & m; r.y.w[q] |= t[24 * e + 12 + q] & m; }
  }
  return r;
}
// acc + (the digit of nibble `nib`) * (the row's point): a mixed addition whatever the digit, kept where the digit is not 0
ECS_HD p384_point p384_add_row(const p384_point& acc, const uint32_t* __restrict__ row, uint32_t nib) {
  uint32_t neg;
  const uint32_t mag = p384_digit_mag(nib, neg);
  p384_affine t = p384_row_select(row, mag);
  t.y = fe384_select(neg, fe384_neg(t.y), t.y);
  return p384_select(p384_eq_mask(mag, 0u), acc, p384_add_mixed(acc, t));
}
// d >> (4 r) for r = 0 .. 3, and the low nibble with a shift by 16 bits: digit 4 j + r of pass r
ECS_HD fe384 p384_pass_digits(const fe384& d, int r) {
  fe384 w;
#pragma unroll
  for (int i = 0; i < 12; ++i) w.w[i] = (uint32_t)((((uint64_t)(i < 11 ? d.w[i < 11 ? i + 1 : 0] : 0u) << 32) | d.w[i]) >> (4 * r));
  return w;
}
ECS_HD uint32_t p384_next_pass_digit(fe384& w) {
  const uint32_t nib = w.w[0] & 15u;
#pragma unroll
  for (int i = 0; i < 11; ++i) w.w[i] = (w.w[i] >> 16) | (w.w[i + 1] << 16);
  w.w[11] >>= 16;
  return nib;
}
// k G for k < n (any k < 2^384 gives k G all the same): sum over r of 16^r sum over j of digit(4 j + r) 65536^j G, by Horner's rule in r
ECS_HD p384_point p384_base_ct(const fe384& k, const uint32_t* __restrict__ base) {
  const p384_digits dg = p384_recode(k);
  p384_point acc = p384_identity();
#pragma unroll 1
  for (int r = 3; r >= 0; --r) {
    fe384 w = p384_pass_digits(dg.d, r);
#pragma unroll 1
    for (int j = 0; j < 24; ++j) acc = p384_add_row(acc, base + (size_t)j * (P384_BASE_ENTRIES * 24), p384_next_pass_digit(w));
    if (r != 0) {                                                                // the pass counter: public
#pragma unroll 1
      for (int d = 0; d < 4; ++d) acc = p384_dbl(acc);
    }
  }
  return p384_add_row(acc, base + (size_t)24 * (P384_BASE_ENTRIES * 24), 8u + dg.c);    // c 16^96 G = c 65536^24 G: the digit c as a nibble
}

// ---- the lane's table of 1 .. 8 P
ECS_HD void p384_table_store(uint32_t* __restrict__ table, size_t lanes, size_t i, int e, const p384_point& p) {
#pragma unroll
  for (int q = 0; q < 12; ++q) {
    table[((size_t)(e * 36 + q)) * lanes + i] = p.X.w[q];
    table[((size_t)(e * 36 + 12 + q)) * lanes + i] = p.Y.w[q];
    table[((size_t)(e * 36 + 24 + q)) * lanes + i] = p.Z.w[q];
  }
}
ECS_HD void p384_table_build(uint32_t* __restrict__ table, size_t lanes, size_t i, const p384_point& p) {
  const p384_point p2 = p384_dbl(p);
  p384_table_store(table, lanes, i, 0, p);
  p384_table_store(table, lanes, i, 1, p2);
  p384_point t = p2;
#pragma unroll 1
  for (int e = 2; e < 8; ++e) { t = p384_add(t, p); p384_table_store(table, lanes, i, e, t); }
}
// +-(mag) P from the table, the identity for mag = 0: every entry read
ECS_HD p384_point p384_table_select(const uint32_t* __restrict__ table, size_t lanes, size_t i, uint32_t nib) {
  uint32_t neg;
  const uint32_t mag = p384_digit_mag(nib, neg);
  p384_point r = {fe384_small(0u), fe384_small(0u), fe384_small(0u)};
#pragma unroll 1                                                                 // one entry in flight (36 words), not all 288: the addresses are e's and the lane's
  for (int e = 0; e < 8; ++e) {
    const uint32_t m = p384_eq_mask(mag, (uint32_t)e + 1u);
#pragma unroll
    for (int q = 0; q < 12; ++q) {
      r.X.w[q] |= table[((size_t)(e * 36 + q)) * lanes + i] & m;
      r.Y.w[q] |= table[((size_t)(e * 36 + 12 + q)) * lanes + i] & m;
      r.Z.w[q] |= table[((size_t)(e * 36 + 24 + q)) * lanes + i] & m;
    }
  }
  r.Y.w[0] |= p384_eq_mask(mag, 0u) & 1u;                                        // (0 : 1 : 0)
  r.Y = fe384_select(neg, fe384_neg(r.Y), r.Y);
  return r;
}
// k P for k < n from the lane's table
ECS_HD p384_point p384_var_ct(const fe384& k, const uint32_t* __restrict__ table, size_t lanes, size_t i) {
  p384_digits dg = p384_recode(k);
  p384_point acc = p384_table_select(table, lanes, i, 8u + dg.c);
#pragma unroll 1
  for (int w = 0; w < 96; ++w) {
#pragma unroll 1
    for (int d = 0; d < 4; ++d) acc = p384_dbl(acc);
    acc = p384_add(acc, p384_table_select(table, lanes, i, p384_top_nibble(dg.d)));
  }
  return acc;
}
// u1 G + u2 Q for u1, u2 < n: Straus, Q's multiples from the lane's table, G's from row 0 of the comb's
ECS_HD p384_point p384_double_mult(const fe384& u1, const fe384& u2, const uint32_t* __restrict__ base, const uint32_t* __restrict__ table, size_t lanes, size_t i) {
  p384_digits d1 = p384_recode(u1), d2 = p384_recode(u2);
  p384_point acc = p384_add_row(p384_table_select(table, lanes, i, 8u + d2.c), base, 8u + d1.c);
#pragma unroll 1
  for (int w = 0; w < 96; ++w) {
#pragma unroll 1
    for (int d = 0; d < 4; ++d) acc = p384_dbl(acc);
    acc = p384_add_row(acc, base, p384_top_nibble(d1.d));
    acc = p384_add(acc, p384_table_select(table, lanes, i, p384_top_nibble(d2.d)));
  }
  return acc;
}

// mask: x(R) mod n = r for 1 <= r < n, without leaving projective form: R is not the identity and r Z = X, or r + n < p and (r + n) Z = X
ECS_HD uint32_t p384_x_equals_mod_n(const p384_point& R, const fe384& r) {
  fe384 rn;
  (void)w384_add(rn, r, fe384_const<p384_consts::N>());                         // used only where r < p - n: no carry there
  const uint32_t second = w384_less(r, fe384_const<p384_consts::P_MINUS_N>());
  const uint32_t hit = fe384_equal(fe384_mul(r, R.Z), R.X) | (second & fe384_equal(fe384_mul(fe384_canon(rn), R.Z), R.X));
  return hit & ~p384_is_identity(R);
}
// mask: 1 <= a < n
ECS_HD uint32_t sc384_in_range(const fe384& a) { return w384_less(a, fe384_const<p384_consts::N>()) & ~fe384_is_zero(a); }

}  // namespace ecsimd_hip
