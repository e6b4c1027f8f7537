// g2.cuh -- the group E'(Fp2): y^2 = x^3 + 4 (1 + u) of BLS12-381 on fp2.cuh, and the standard encodings' rules.  PUBLIC data only: every exceptional case of
// the group law, every validity test and every scalar bit is a branch.
//
// Points: Jacobian (X : Y : Z), x = X / Z^2, y = Y / Z^3, coordinates canonical (fp2.cuh); Z = 0 is the identity, whatever X and Y hold.  a = 0.  The three
// operations take g1.cuh's decisions:
//   g2_dbl   2 P for EVERY P (2M + 5S in Fp2): Z = 0 stays Z = 0, and so does Y = 0 (E'(Fp2) has no such point -- its order h2 r is odd -- but the code does not
//            lean on that: the host check doubles one made by hand).
//   g2_add   P + Q for every P, Q (12M + 4S): either at infinity, P = Q (H = 0 and r = 0: the tangent), P = -Q (H = 0 only: the identity).
//   g2_madd  P + (x2, y2) for every Jacobian P and every FINITE affine point (8M + 3S), behind the same decisions.
// G2_OP is what the three are declared with: __host__ __device__ __forceinline__ unless the including unit says otherwise (k_bls12_381_g2.hip keeps them out of
// line: one copy of each in the unit, see its head).
//
// g2_mul: k P for a public 256-bit k and an affine P, left-to-right double-and-add with MIXED additions, over the INTEGERS: P need not lie in G2.
// g2_in_subgroup is the definition, [r] P = identity, by the same loop (the cofactor h2 has 507 bits: almost no point of E'(Fp2) is in G2).
//
// WIRE ORDER: c1 BEFORE c0 (x.c1 || x.c0 || y.c1 || y.c0), the flag bits in the first byte of x.c1; the lexicographic rule is fp2_lex_largest.
#pragma once
#include "fp2.cuh"

#ifndef G2_OP
#define G2_OP ECS_HD
#endif

namespace ecsimd_hip {

struct g2_point { fp2 x, y, z; };
struct g2_affine { fp2 x, y; };                                       // finite, Montgomery form

// the group order r, 255 bits, as eight words (g1.cuh's ORDER: the two groups have the same order)
struct g2_consts { static constexpr uint32_t ORDER[8] = {0x00000001u, 0xffffffffu, 0xfffe5bfeu, 0x53bda402u, 0x09a1d805u, 0x3339d808u, 0x299d7d48u, 0x73eda753u}; };

ECS_HD fp2 g2_b() { return {fe384_const<bls381_consts::B4>(), fe384_const<bls381_consts::B4>()}; }   // 4 + 4 u
ECS_HD g2_point g2_identity() { g2_point R; R.x = fp2_zero(); R.y = fp2_zero(); R.z = fp2_zero(); return R; }
ECS_HD bool g2_is_identity(const g2_point& P) { return fp2_is_zero(P.z); }
ECS_HD g2_point g2_from_affine(const g2_affine& a) { g2_point R; R.x = a.x; R.y = a.y; R.z = fp2_one(); return R; }
ECS_HD g2_point g2_neg(const g2_point& P) { g2_point R = P; R.y = fp2_neg(P.y); return R; }
ECS_HD bool g2_on_curve(const fp2& x, const fp2& y) { return fp2_equal(fp2_sqr(y), fp2_add(fp2_mul(fp2_sqr(x), x), g2_b())); }

G2_OP g2_point g2_dbl(const g2_point& P) {
  const fp2 YY = fp2_sqr(P.y);
  const fp2 S = fp2_dbl(fp2_dbl(fp2_mul(P.x, YY)));
  const fp2 XX = fp2_sqr(P.x);
  const fp2 M = fp2_add(fp2_dbl(XX), XX);
  g2_point R;
  R.x = fp2_sub(fp2_sqr(M), fp2_dbl(S));
  R.z = fp2_dbl(fp2_mul(P.y, P.z));
  R.y = fp2_sub(fp2_mul(M, fp2_sub(S, R.x)), fp2_dbl(fp2_dbl(fp2_dbl(fp2_sqr(YY)))));
  return R;
}
G2_OP g2_point g2_add(const g2_point& P, const g2_point& Q) {
  if (fp2_is_zero(P.z)) return Q;
  if (fp2_is_zero(Q.z)) return P;
  const fp2 Z1Z1 = fp2_sqr(P.z), Z2Z2 = fp2_sqr(Q.z);
  const fp2 U1 = fp2_mul(P.x, Z2Z2), U2 = fp2_mul(Q.x, Z1Z1);
  const fp2 S1 = fp2_mul(P.y, fp2_mul(Q.z, Z2Z2)), S2 = fp2_mul(Q.y, fp2_mul(P.z, Z1Z1));
  const fp2 H = fp2_sub(U2, U1), r = fp2_sub(S2, S1);
  if (fp2_is_zero(H)) return fp2_is_zero(r) ? g2_dbl(P) : g2_identity();
  const fp2 HH = fp2_sqr(H), HHH = fp2_mul(H, HH), V = fp2_mul(U1, HH);
  g2_point R;
  R.x = fp2_sub(fp2_sub(fp2_sqr(r), HHH), fp2_dbl(V));
  R.y = fp2_sub(fp2_mul(r, fp2_sub(V, R.x)), fp2_mul(S1, HHH));
  R.z = fp2_mul(fp2_mul(P.z, Q.z), H);
  return R;
}
G2_OP g2_point g2_madd(const g2_point& P, const g2_affine& Q) {
  if (fp2_is_zero(P.z)) return g2_from_affine(Q);
  const fp2 Z1Z1 = fp2_sqr(P.z);
  const fp2 H = fp2_sub(fp2_mul(Q.x, Z1Z1), P.x), r = fp2_sub(fp2_mul(Q.y, fp2_mul(Z1Z1, P.z)), P.y);
  if (fp2_is_zero(H)) return fp2_is_zero(r) ? g2_dbl(g2_from_affine(Q)) : g2_identity();
  const fp2 HH = fp2_sqr(H), HHH = fp2_mul(H, HH), V = fp2_mul(P.x, HH);
  g2_point R;
  R.z = fp2_mul(P.z, H);
  R.x = fp2_sub(fp2_sub(fp2_sqr(r), HHH), fp2_dbl(V));
  R.y = fp2_sub(fp2_mul(r, fp2_sub(V, R.x)), fp2_mul(P.y, HHH));
  return R;
}
// the affine point of a FINITE P: one inversion
ECS_HD g2_affine g2_to_affine(const g2_point& P) {
  const fp2 iz = fp2_invert(P.z), iz2 = fp2_sqr(iz);
  return {fp2_mul(P.x, iz2), fp2_mul(P.y, fp2_mul(iz2, iz))};
}

// k P for the eight little-endian words of a public k (see the head of the file)
ECS_HD g2_point g2_mul(const uint32_t (&k)[8], const g2_affine& P) {
  g2_point acc = g2_identity();
#pragma unroll 1
  for (int w = 7; w >= 0; --w) {
    uint32_t e = 0;
#pragma unroll
    for (int q = 0; q < 8; ++q) e = w == q ? k[q] : e;
#pragma unroll 1
    for (int b = 31; b >= 0; --b) {
      acc = g2_dbl(acc);
      if ((e >> b) & 1u) acc = g2_madd(acc, P);
    }
  }
  return acc;
}
// [r] P is the identity: THE DEFINITION of membership in G2
ECS_HD bool g2_in_subgroup(const g2_affine& P) {
  uint32_t k[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) k[q] = g2_consts::ORDER[q];
  return g2_is_identity(g2_mul(k, P));
}

// ---- the serialisation's rules on plain big-endian-decoded words (w[11] holds byte 0 .. 3 of a 48-byte component), in WIRE order: c1 first.  Results: 0 the
// identity, 1 a point (x, y in Montgomery form), 2 malformed.
constexpr int G2_INFINITY = 0, G2_POINT = 1, G2_MALFORMED = 2;
ECS_HD bool g2_words_zero(const fe381& a, uint32_t top_mask) {
  uint32_t d = a.w[11] & top_mask;
#pragma unroll
  for (int i = 0; i < 11; ++i) d |= a.w[i];
  return d == 0u;
}
// uncompressed: x.c1, x.c0, y.c1, y.c0 as read; flags are the top three bits of x.c1 (a flag bit in any other component makes it >= p)
ECS_HD int g2_decode192(const fe381& x1w, const fe381& x0w, const fe381& y1w, const fe381& y0w, g2_affine& out) {
  const uint32_t flags = x1w.w[11] >> 29;
  out.x = fp2_zero(); out.y = fp2_zero();
  if (flags == 2u)
    return (g2_words_zero(x1w, 0x1fffffffu) && g2_words_zero(x0w, 0xffffffffu) && g2_words_zero(y1w, 0xffffffffu) && g2_words_zero(y0w, 0xffffffffu)) ? G2_INFINITY : G2_MALFORMED;
  if (flags != 0u || !fe381_below_p(x1w) || !fe381_below_p(x0w) || !fe381_below_p(y1w) || !fe381_below_p(y0w)) return G2_MALFORMED;
  const fp2 x = fp2_to_mont(x0w, x1w), y = fp2_to_mont(y0w, y1w);
  if (!g2_on_curve(x, y)) return G2_MALFORMED;
  out.x = x; out.y = y;
  return G2_POINT;
}
// compressed: x.c1 (flags in its top three bits), x.c0 as read
ECS_HD int g2_decode96(const fe381& c1w, const fe381& c0w, g2_affine& out) {
  const uint32_t flags = c1w.w[11] >> 29;
  out.x = fp2_zero(); out.y = fp2_zero();
  if (!(flags & 4u)) return G2_MALFORMED;
  if (flags & 2u) return (flags == 6u && g2_words_zero(c1w, 0x1fffffffu) && g2_words_zero(c0w, 0xffffffffu)) ? G2_INFINITY : G2_MALFORMED;
  fe381 x1w = c1w; x1w.w[11] &= 0x1fffffffu;
  if (!fe381_below_p(x1w) || !fe381_below_p(c0w)) return G2_MALFORMED;
  const fp2 x = fp2_to_mont(c0w, x1w);
  bool ok;
  fp2 y = fp2_sqrt(fp2_add(fp2_mul(fp2_sqr(x), x), g2_b()), ok);
  if (!ok) return G2_MALFORMED;
  if (fp2_lex_largest(y) != ((flags & 1u) != 0u)) y = fp2_neg(y);
  out.x = x; out.y = y;
  return G2_POINT;
}
// the plain words of the two encodings of a point (cls: G2_INFINITY or G2_POINT), in wire order
ECS_HD void g2_encode192(int cls, const g2_affine& a, fe381& x1w, fe381& x0w, fe381& y1w, fe381& y0w) {
  x1w = fe381_zero(); x0w = fe381_zero(); y1w = fe381_zero(); y0w = fe381_zero();
  if (cls == G2_INFINITY) { x1w.w[11] = 0x40000000u; return; }
  fp2_from_mont(a.x, x0w, x1w); fp2_from_mont(a.y, y0w, y1w);
}
ECS_HD void g2_encode96(int cls, const g2_affine& a, fe381& c1w, fe381& c0w) {
  c1w = fe381_zero(); c0w = fe381_zero();
  if (cls == G2_INFINITY) { c1w.w[11] = 0xc0000000u; return; }
  fp2_from_mont(a.x, c0w, c1w);
  c1w.w[11] |= 0x80000000u | (fp2_lex_largest(a.y) ? 0x20000000u : 0u);
}

}  // namespace ecsimd_hip
