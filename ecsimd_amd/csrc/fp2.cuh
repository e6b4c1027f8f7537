// fp2.cuh -- the quadratic extension Fp2 = Fp[u] / (u^2 + 1) of the BLS12-381 base field, on fe381.cuh, one element per lane.
//
// REPRESENTATION: a = c0 + c1 u, BOTH components canonical Montgomery-form values of fe381.cuh (below p), always.  So equality is a comparison of 24 words,
// "is zero" is 24 ORs, and g2.cuh's exceptional cases (decided on H = 0 and r = 0) are exact without a normalisation.
//
// PRODUCT: KARATSUBA on three Fp products, each reduced (not the lazy form with two reductions of 24-word sums: fe381.cuh keeps everything canonical and has
// no 768-bit addition; nobody has measured the lazy form here).  By the source:
//   fp2_mul   t0 = a0 b0, t1 = a1 b1, t2 = (a0 + a1)(b0 + b1); c0 = t0 - t1, c1 = t2 - t0 - t1: 3 x 288 = 864 multiply-adds, two additions, three subtractions.
//   fp2_sqr   c0 = (a0 + a1)(a0 - a1), c1 = 2 a0 a1: 2 x 288 = 576 multiply-adds (the complex squaring; no fe381_sqr in it), two additions, one subtraction.
// tools/bls12_381_listing.py --unit g2 reports what the compiler makes of them.
//
// fp2_invert is ONE Fp inversion, of the norm a0^2 + a1^2 (non-zero for a != 0 because -1 is no square modulo p = 3 mod 4): 1 / a = conj(a) / norm.  0 -> 0.
// fp2_sqrt returns a root whenever one exists and says so when none does; BOTH are decided by squaring the candidate.  With n = a0^2 + a1^2 (a square of Fp
// exactly when a is a square of Fp2) and s = sqrt(n): exactly one of 2 (a0 + s) and 2 (a0 - s) is a square of Fp for a1 != 0 (their product is -4 a1^2); with t
// its root the candidate is (t / 2, a1 / t), both through ONE inversion w = 1 / (2 t): (t^2 w, 2 a1 w).  An input IN Fp (a1 = 0) takes a branch of its own -- the
// alpha = -1 branch of the usual p = 3 mod 4 algorithm: a residue a0 has the real root (sqrt(a0), 0), a non-residue the purely imaginary (0, sqrt(-a0)).
// Branches on data: this layer is for PUBLIC data only, like g1.cuh and g2.cuh above it.
//
// Every function is __host__ __device__, so tests/cpp/bls12_381_g2_host_check.cpp runs this very text on a CPU.
#pragma once
#include "fe381.cuh"

namespace ecsimd_hip {

struct fp2 { fe381 c0, c1; };                                         // c0 + c1 u

ECS_HD fp2 fp2_zero() { return {fe381_zero(), fe381_zero()}; }
ECS_HD fp2 fp2_one() { return {fe381_one(), fe381_zero()}; }
ECS_HD bool fp2_is_zero(const fp2& a) { return fe381_is_zero(a.c0) && fe381_is_zero(a.c1); }
ECS_HD bool fp2_equal(const fp2& a, const fp2& b) { return fe381_equal(a.c0, b.c0) && fe381_equal(a.c1, b.c1); }
ECS_HD fp2 fp2_add(const fp2& a, const fp2& b) { return {fe381_add(a.c0, b.c0), fe381_add(a.c1, b.c1)}; }
ECS_HD fp2 fp2_sub(const fp2& a, const fp2& b) { return {fe381_sub(a.c0, b.c0), fe381_sub(a.c1, b.c1)}; }
ECS_HD fp2 fp2_neg(const fp2& a) { return {fe381_neg(a.c0), fe381_neg(a.c1)}; }
ECS_HD fp2 fp2_dbl(const fp2& a) { return {fe381_dbl(a.c0), fe381_dbl(a.c1)}; }
ECS_HD fp2 fp2_conj(const fp2& a) { return {a.c0, fe381_neg(a.c1)}; }
ECS_HD fp2 fp2_mul(const fp2& a, const fp2& b) {
  const fe381 t0 = fe381_mul(a.c0, b.c0), t1 = fe381_mul(a.c1, b.c1);
  const fe381 t2 = fe381_mul(fe381_add(a.c0, a.c1), fe381_add(b.c0, b.c1));
  return {fe381_sub(t0, t1), fe381_sub(fe381_sub(t2, t0), t1)};
}
ECS_HD fp2 fp2_sqr(const fp2& a) {
  const fe381 c0 = fe381_mul(fe381_add(a.c0, a.c1), fe381_sub(a.c0, a.c1));
  return {c0, fe381_dbl(fe381_mul(a.c0, a.c1))};
}
ECS_HD fp2 fp2_mul_fp(const fp2& a, const fe381& s) { return {fe381_mul(a.c0, s), fe381_mul(a.c1, s)}; }
// any two 384-bit values -> the element; and back to plain residues below p
ECS_HD fp2 fp2_to_mont(const fe381& v0, const fe381& v1) { return {fe381_to_mont(v0), fe381_to_mont(v1)}; }
ECS_HD void fp2_from_mont(const fp2& a, fe381& v0, fe381& v1) { v0 = fe381_from_mont(a.c0); v1 = fe381_from_mont(a.c1); }
ECS_HD fp2 fp2_invert(const fp2& a) {                                 // 0 -> 0
  const fe381 inv = fe381_invert(fe381_add(fe381_sqr(a.c0), fe381_sqr(a.c1)));
  return {fe381_mul(a.c0, inv), fe381_neg(fe381_mul(a.c1, inv))};
}
// a square root of a, and whether a has one (see the head of the file)
ECS_HD fp2 fp2_sqrt(const fp2& a, bool& ok) {
  fp2 cand = fp2_zero();
  bool have;
  if (fe381_is_zero(a.c1)) {
    const fe381 s = fe381_sqrt(a.c0, have);
    if (have) cand.c0 = s;
    else cand.c1 = fe381_sqrt(fe381_neg(a.c0), have);                 // -1 is a non-residue: exactly one of a0, -a0 has a root
  } else {
    const fe381 s = fe381_sqrt(fe381_add(fe381_sqr(a.c0), fe381_sqr(a.c1)), have);
    if (have) {
      fe381 t = fe381_sqrt(fe381_dbl(fe381_add(a.c0, s)), have);
      if (!have) t = fe381_sqrt(fe381_dbl(fe381_sub(a.c0, s)), have);
      const fe381 w = fe381_invert(fe381_dbl(t));
      cand.c0 = fe381_mul(fe381_sqr(t), w);
      cand.c1 = fe381_mul(fe381_dbl(a.c1), w);
    }
  }
  ok = fp2_equal(fp2_sqr(cand), a);
  return cand;
}
// "lexicographically largest" of the serialisation: c1 > (p - 1) / 2, or c1 = 0 and c0 > (p - 1) / 2
ECS_HD bool fp2_lex_largest(const fp2& a) { return fe381_is_zero(a.c1) ? fe381_lex_largest(a.c0) : fe381_lex_largest(a.c1); }

}  // namespace ecsimd_hip
