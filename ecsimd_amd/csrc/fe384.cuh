// fe384.cuh -- arithmetic modulo p = 2^384 - 2^128 - 2^96 + 2^32 - 1 (NIST P-384) and modulo the group order n, one element per lane.
//
// Representation: twelve saturated 32-bit words in registers, PLAIN residues, always canonical (below p): every function takes canonical operands and returns
// a canonical result, so equality is a comparison of words and the wire format is the words.  fe384_canon takes any 384-bit value (2^384 < 2 p: one
// conditional subtraction); that is the load rule for raw inputs.
//
// Product and squaring: Comba columns with v_mad_u64_u32 in field.cuh's ECS_MAC style (mac_col), 144 multiply-adds for the product; a column longer than
// eight products is two mac_col statements.  The squaring takes each cross product once (66) and doubles the column's cross sum before the square (12) goes
// on top: 78 multiply-adds.
//
// REDUCTION: FIPS 186-4 D.2.4, the Solinas folding of the 768-bit product on plain residues -- chosen over Montgomery with R = 2^384.  Both cost no
// multiplication (-1/p mod 2^32 = 1 makes every Montgomery quotient digit the raw column word, and q p is q shifted by 0, 1, 3, 4 and 12 words), but the
// Montgomery form serialises twelve dependent passes of a five-term signed carry chain over up to thirteen words behind the columns, and every value that
// crosses the wire pays a conversion; the folding is ONE pass of twelve signed 64-bit column sums (62 word terms in all: T + 2 S1 + S2 + .. + S6 - D1 - D2 - D3),
// two short folds of the signed carry word (it lies in [-1, 3]; 2^384 = 2^128 + 2^96 - 2^32 + 1) and one conditional subtraction of p, and constants, table
// entries and wire values are used as they are.  From the shipped listing (profiles/r18/p384_listing.json, tools/p384_listing.py): one complete addition --
// 14 products, 23 additions and subtractions -- is 2 016 v_mad_u64_u32 and 11 610 VALU instructions in all, 2 388 of them moves: 5.76 VALU per multiply-add,
// of which 2 are the column statement's own (the multiply-add and its carry word); the rest is the folding, the masked corrections and the moves.
// Nobody has compared a reduced-radix representation (29-bit style limbs) with this on twelve words.
//
// No branch on data anywhere: conditional subtractions and selections go by masks, so the secret kernels of k_p384.hip use this layer as it is.
//
// Scalars modulo n: n is dense, so the product is a word-serial Montgomery product (gfield.cuh's algorithm at twelve words) on values in Montgomery form
// inside sc384_mul / sc384_invert; operands and results of the public functions are plain.  Inversion is a^(n - 2) with the bits of the PUBLIC exponent as
// loop constants: the same instruction sequence for every operand, which is what signing's secret k needs.
//
// Every function is __host__ __device__: on the host the column multiply-add is plain C++ (fe384_mac), so a CPU program can run the very same reduction,
// group law and window loops against big integers (tests/cpp/p384_host_check.cpp).
#pragma once
#include "field.cuh"
#include "p384_base.inc"

namespace ecsimd_hip {

#define ECS_HD __host__ __device__ __forceinline__

struct fe384 { uint32_t w[12]; };
struct fe768 { uint32_t w[24]; };

struct p384_consts {
  static constexpr uint32_t P[12] = P384_P_WORDS;
  static constexpr uint32_t N[12] = P384_N_WORDS;
  static constexpr uint32_t B[12] = P384_B_WORDS;
  static constexpr uint32_t N_MINUS_2[12] = P384_N_MINUS_2_WORDS;
  static constexpr uint32_t N_R2[12] = P384_N_R2_WORDS;               // 2^768 mod n
  static constexpr uint32_t P_MINUS_N[12] = P384_P_MINUS_N_WORDS;     // r + n < p  <=>  r < p - n
};
template <const uint32_t (&ARR)[12]> ECS_HD fe384 fe384_const() {
  fe384 r;
#pragma unroll
  for (int i = 0; i < 12; ++i) r.w[i] = ARR[i];
  return r;
}
ECS_HD fe384 fe384_small(uint32_t v) {
  fe384 r;
  r.w[0] = v;
#pragma unroll
  for (int i = 1; i < 12; ++i) r.w[i] = 0u;
  return r;
}

// ---- words: carries, borrows, masks.  A mask is 0 or 0xffffffff.
ECS_HD uint32_t w384_add(fe384& r, const fe384& a, const fe384& b) {            // returns the carry, 0 or 1
  uint64_t acc = 0;
#pragma unroll
  for (int i = 0; i < 12; ++i) { acc += (uint64_t)a.w[i] + b.w[i]; r.w[i] = (uint32_t)acc; acc >>= 32; }
  return (uint32_t)acc;
}
ECS_HD uint32_t w384_sub(fe384& r, const fe384& a, const fe384& b) {            // returns the borrow as a mask
  int64_t acc = 0;
#pragma unroll
  for (int i = 0; i < 12; ++i) { acc += (int64_t)a.w[i] - (int64_t)b.w[i]; r.w[i] = (uint32_t)acc; acc >>= 32; }
  return (uint32_t)acc;
}
ECS_HD fe384 fe384_select(uint32_t mask, const fe384& a, const fe384& b) {      // mask ? a : b
  fe384 r;
#pragma unroll
  for (int i = 0; i < 12; ++i) r.w[i] = (a.w[i] & mask) | (b.w[i] & ~mask);
  return r;
}
ECS_HD uint32_t mask384_nonzero(uint32_t v) { return (uint32_t)((int32_t)(v | (0u - v)) >> 31); }
ECS_HD uint32_t fe384_is_zero(const fe384& a) {                                 // mask; a canonical
  uint32_t d = 0;
#pragma unroll
  for (int i = 0; i < 12; ++i) d |= a.w[i];
  return ~mask384_nonzero(d);
}
ECS_HD uint32_t fe384_equal(const fe384& a, const fe384& b) {
  uint32_t d = 0;
#pragma unroll
  for (int i = 0; i < 12; ++i) d |= a.w[i] ^ b.w[i];
  return ~mask384_nonzero(d);
}
ECS_HD uint32_t w384_less(const fe384& a, const fe384& b) { fe384 t; return w384_sub(t, a, b); }    // mask: a < b as integers

// r (+ 2^384 where carry is a full mask) minus M where that is not negative: the one conditional subtraction behind an addition or a fold
template <const uint32_t (&M)[12]> ECS_HD fe384 w384_cond_sub(const fe384& r, uint32_t carry_mask) {
  fe384 t;
  const uint32_t borrow = w384_sub(t, r, fe384_const<M>());
  return fe384_select(carry_mask | ~borrow, t, r);
}
template <const uint32_t (&M)[12]> ECS_HD fe384 mod384_add(const fe384& a, const fe384& b) {
  fe384 r;
  const uint32_t c = w384_add(r, a, b);
  return w384_cond_sub<M>(r, 0u - c);
}
template <const uint32_t (&M)[12]> ECS_HD fe384 mod384_sub(const fe384& a, const fe384& b) {
  fe384 r, m = fe384_const<M>();
  const uint32_t borrow = w384_sub(r, a, b);
#pragma unroll
  for (int i = 0; i < 12; ++i) m.w[i] &= borrow;
  (void)w384_add(r, r, m);
  return r;
}

ECS_HD fe384 fe384_canon(const fe384& a) { return w384_cond_sub<p384_consts::P>(a, 0u); }
ECS_HD fe384 fe384_add(const fe384& a, const fe384& b) { return mod384_add<p384_consts::P>(a, b); }
ECS_HD fe384 fe384_sub(const fe384& a, const fe384& b) { return mod384_sub<p384_consts::P>(a, b); }
ECS_HD fe384 fe384_neg(const fe384& a) { return mod384_sub<p384_consts::P>(fe384_small(0u), a); }
ECS_HD fe384 fe384_dbl(const fe384& a) { return fe384_add(a, a); }

// ---- 384 x 384 -> 768: Comba columns.  acc += sum a[i] b[i], ex = the carries out of the 64-bit accumulator.
template <int N> ECS_HD void fe384_mac(uint64_t& acc, uint32_t& ex, const uint32_t (&a)[N], const uint32_t (&b)[N]) {
#if defined(__HIP_DEVICE_COMPILE__)
  mac_col<N>(acc, ex, a, b);
#else
  ex = 0;
  for (int i = 0; i < N; ++i) { const uint64_t p = (uint64_t)a[i] * b[i]; acc += p; ex += acc < p ? 1u : 0u; }
#endif
}
// column K of a b: the products a[i] b[K - i]
template <int K> ECS_HD void mul384_col(uint64_t& acc, uint32_t& ex, const fe384& a, const fe384& b) {
  constexpr int lo = K > 11 ? K - 11 : 0, hi = K < 11 ? K : 11, N = hi - lo + 1, N1 = N > 8 ? 8 : N, N2 = N - N1;
  uint32_t x[N1], y[N1];
#pragma unroll
  for (int i = 0; i < N1; ++i) { x[i] = a.w[lo + i]; y[i] = b.w[K - lo - i]; }
  fe384_mac<N1>(acc, ex, x, y);
  if constexpr (N2 > 0) {
    uint32_t x2[N2], y2[N2], ex2;
#pragma unroll
    for (int i = 0; i < N2; ++i) { x2[i] = a.w[lo + 8 + i]; y2[i] = b.w[K - lo - 8 - i]; }
    fe384_mac<N2>(acc, ex2, x2, y2);
    ex += ex2;
  }
}
template <int K> ECS_HD void mul384_cols(fe768& t, uint64_t& acc, const fe384& a, const fe384& b) {
  if constexpr (K < 23) {
    uint32_t ex;
    mul384_col<K>(acc, ex, a, b);
    t.w[K] = (uint32_t)acc;
    acc = (acc >> 32) | ((uint64_t)ex << 32);
    mul384_cols<K + 1>(t, acc, a, b);
  }
}
ECS_HD fe768 mul12x12(const fe384& a, const fe384& b) {
  fe768 t;
  uint64_t acc = 0;
  mul384_cols<0>(t, acc, a, b);
  t.w[23] = (uint32_t)acc;
  return t;
}
// column K of a^2: twice the cross products a[i] a[K - i], i < K - i, and the square of the middle word where K is even
template <int K> ECS_HD void sqr384_cols(fe768& t, uint64_t& acc, const fe384& a) {
  if constexpr (K < 23) {
    constexpr int lo = K > 11 ? K - 11 : 0, N = (K + 1) / 2 - lo;                // cross products: i = lo .. lo + N - 1
    uint32_t top = 0;                                                          // the column's bits 64 .. 95
    if constexpr (N > 0) {
      uint64_t cross = 0;
      uint32_t cex, x[N], y[N];
#pragma unroll
      for (int i = 0; i < N; ++i) { x[i] = a.w[lo + i]; y[i] = a.w[K - lo - i]; }
      fe384_mac<N>(cross, cex, x, y);
      top = (cex << 1) | (uint32_t)(cross >> 63);
      cross <<= 1;
      acc += cross;
      top += acc < cross ? 1u : 0u;
    }
    if constexpr (K % 2 == 0) {
      uint32_t sex;
      const uint32_t m[1] = {a.w[K / 2]};
      fe384_mac<1>(acc, sex, m, m);
      top += sex;
    }
    t.w[K] = (uint32_t)acc;
    acc = (acc >> 32) | ((uint64_t)top << 32);
    sqr384_cols<K + 1>(t, acc, a);
  }
}
ECS_HD fe768 sqr12(const fe384& a) {
  fe768 t;
  uint64_t acc = 0;
  sqr384_cols<0>(t, acc, a);
  t.w[23] = (uint32_t)acc;
  return t;
}

// r + c (2^128 + 2^96 - 2^32 + 1) for a small signed c: 2^384 c folded in; returns the new signed carry
ECS_HD int32_t fe384_fold_carry(fe384& r, int32_t c) {
  int64_t acc = (int64_t)r.w[0] + c;
  r.w[0] = (uint32_t)acc; acc >>= 32;
  acc += (int64_t)r.w[1] - c; r.w[1] = (uint32_t)acc; acc >>= 32;
  acc += (int64_t)r.w[2]; r.w[2] = (uint32_t)acc; acc >>= 32;
  acc += (int64_t)r.w[3] + c; r.w[3] = (uint32_t)acc; acc >>= 32;
  acc += (int64_t)r.w[4] + c; r.w[4] = (uint32_t)acc; acc >>= 32;
#pragma unroll
  for (int i = 5; i < 12; ++i) { acc += (int64_t)r.w[i]; r.w[i] = (uint32_t)acc; acc >>= 32; }
  return (int32_t)acc;
}
// the 768-bit t modulo p (FIPS 186-4 D.2.4): column sums of T + 2 S1 + S2 + S3 + S4 + S5 + S6 - D1 - D2 - D3 with a signed carry, the carry word (in
// [-1, 3] whatever the 24 words are) folded -- the value is then within 2^132 of [0, 2^384), so the second fold's carry is -1, 0 or 1 and the third's 0 --,
// then one conditional subtraction.
ECS_HD fe384 fe384_reduce(const fe768& t) {
  fe384 r;
  int64_t acc = 0;
#define A(i) (int64_t)t.w[i]
#define ECS_P384_COL(K, EXPR) acc += (EXPR); r.w[K] = (uint32_t)acc; acc >>= 32;
  ECS_P384_COL(0, A(0) + A(12) + A(21) + A(20) - A(23))
  ECS_P384_COL(1, A(1) + A(13) + A(22) + A(23) - A(12) - A(20))
  ECS_P384_COL(2, A(2) + A(14) + A(23) - A(13) - A(21))
  ECS_P384_COL(3, A(3) + A(15) + A(12) + A(20) + A(21) - A(14) - A(22) - A(23))
  ECS_P384_COL(4, A(4) + 2 * A(21) + A(16) + A(13) + A(12) + A(20) + A(22) - A(15) - 2 * A(23))
  ECS_P384_COL(5, A(5) + 2 * A(22) + A(17) + A(14) + A(13) + A(21) + A(23) - A(16))
  ECS_P384_COL(6, A(6) + 2 * A(23) + A(18) + A(15) + A(14) + A(22) - A(17))
  ECS_P384_COL(7, A(7) + A(19) + A(16) + A(15) + A(23) - A(18))
  ECS_P384_COL(8, A(8) + A(20) + A(17) + A(16) - A(19))
  ECS_P384_COL(9, A(9) + A(21) + A(18) + A(17) - A(20))
  ECS_P384_COL(10, A(10) + A(22) + A(19) + A(18) - A(21))
  ECS_P384_COL(11, A(11) + A(23) + A(20) + A(19) - A(22))
#undef ECS_P384_COL
#undef A
  int32_t c = fe384_fold_carry(r, (int32_t)acc);
  c = fe384_fold_carry(r, c);
  (void)c;                                                                     // 0: see above
  return fe384_canon(r);
}
ECS_HD fe384 fe384_mul(const fe384& a, const fe384& b) { return fe384_reduce(mul12x12(a, b)); }
ECS_HD fe384 fe384_sqr(const fe384& a) { return fe384_reduce(sqr12(a)); }
ECS_HD fe384 fe384_sqr_n(fe384 a, int n) {
#pragma unroll 1
  for (int i = 0; i < n; ++i) a = fe384_sqr(a);
  return a;
}
// a^(p - 2) by a fixed chain (0 -> 0).  p - 2 = [255 ones][0][32 ones][64 zeros][30 ones][0][1]: 383 squarings and 14 products.
ECS_HD fe384 fe384_invert(const fe384& a) {
  const fe384 x2 = fe384_mul(fe384_sqr(a), a);
  const fe384 x3 = fe384_mul(fe384_sqr(x2), a);
  const fe384 x6 = fe384_mul(fe384_sqr_n(x3, 3), x3);
  const fe384 x12 = fe384_mul(fe384_sqr_n(x6, 6), x6);
  const fe384 x15 = fe384_mul(fe384_sqr_n(x12, 3), x3);
  const fe384 x30 = fe384_mul(fe384_sqr_n(x15, 15), x15);
  const fe384 x60 = fe384_mul(fe384_sqr_n(x30, 30), x30);
  const fe384 x120 = fe384_mul(fe384_sqr_n(x60, 60), x60);
  const fe384 x240 = fe384_mul(fe384_sqr_n(x120, 120), x120);
  const fe384 x255 = fe384_mul(fe384_sqr_n(x240, 15), x15);
  const fe384 x32 = fe384_mul(fe384_sqr_n(x30, 2), x2);
  fe384 r = fe384_mul(fe384_sqr_n(x255, 33), x32);
  r = fe384_mul(fe384_sqr_n(r, 94), x30);
  return fe384_mul(fe384_sqr_n(r, 2), a);
}

// ---- scalars modulo n
ECS_HD fe384 sc384_reduce(const fe384& a) { return w384_cond_sub<p384_consts::N>(a, 0u); }        // any 384-bit value: 2^384 < 2 n
ECS_HD fe384 sc384_add(const fe384& a, const fe384& b) { return mod384_add<p384_consts::N>(a, b); }
ECS_HD fe384 sc384_sub(const fe384& a, const fe384& b) { return mod384_sub<p384_consts::N>(a, b); }
ECS_HD fe384 sc384_neg(const fe384& a) { return mod384_sub<p384_consts::N>(fe384_small(0u), a); }
// a b / 2^384 mod n, a and b below n: word-serial Montgomery (one word of b, then one quotient digit, per pass)
ECS_HD fe384 sc384_mont(const fe384& a, const fe384& b) {
  uint32_t t[13];
#pragma unroll
  for (int i = 0; i < 13; ++i) t[i] = 0u;
#pragma unroll
  for (int i = 0; i < 12; ++i) {
    uint64_t acc = 0;
#pragma unroll
    for (int j = 0; j < 12; ++j) { acc += (uint64_t)a.w[j] * b.w[i] + t[j]; t[j] = (uint32_t)acc; acc >>= 32; }
    acc += t[12];
    t[12] = (uint32_t)acc;
    const uint32_t t13 = (uint32_t)(acc >> 32);
    const uint32_t m = t[0] * P384_N_NEG_INV32;
    acc = ((uint64_t)m * p384_consts::N[0] + t[0]) >> 32;
#pragma unroll
    for (int j = 1; j < 12; ++j) { acc += (uint64_t)m * p384_consts::N[j] + t[j]; t[j - 1] = (uint32_t)acc; acc >>= 32; }
    acc += t[12];
    t[11] = (uint32_t)acc;
    t[12] = t13 + (uint32_t)(acc >> 32);
  }
  fe384 r;
#pragma unroll
  for (int i = 0; i < 12; ++i) r.w[i] = t[i];
  return w384_cond_sub<p384_consts::N>(r, 0u - t[12]);
}
ECS_HD fe384 sc384_to_mont(const fe384& a) { return sc384_mont(a, fe384_const<p384_consts::N_R2>()); }
ECS_HD fe384 sc384_from_mont(const fe384& a) { return sc384_mont(a, fe384_small(1u)); }
ECS_HD fe384 sc384_mul(const fe384& a, const fe384& b) { return sc384_mont(sc384_mont(a, b), fe384_const<p384_consts::N_R2>()); }
// a^(n - 2) mod n (0 -> 0): square and multiply over the bits of the public exponent, most significant first
ECS_HD fe384 sc384_invert(const fe384& a) {
  const fe384 am = sc384_to_mont(a);
  fe384 r = sc384_to_mont(fe384_small(1u));
#pragma unroll 1
  for (int w = 11; w >= 0; --w) {
    uint32_t e = 0;
#pragma unroll
    for (int q = 0; q < 12; ++q) e = w == q ? p384_consts::N_MINUS_2[q] : e;     // w is a loop counter: uniform selects of literals
#pragma unroll 1
    for (int b = 31; b >= 0; --b) {
      r = sc384_mont(r, r);
      if ((e >> b) & 1u) r = sc384_mont(r, am);                                // a bit of n - 2: public, the same on every lane
    }
  }
  return sc384_from_mont(r);
}

}  // namespace ecsimd_hip
