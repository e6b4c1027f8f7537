// g1.cuh -- the group E(Fp): y^2 = x^3 + 4 of BLS12-381 on fe381.cuh, and the standard encodings' rules.  PUBLIC data only: every exceptional case of the
// group law, every validity test and every scalar bit is a branch.
//
// Points: Jacobian (X : Y : Z), x = X / Z^2, y = Y / Z^3, coordinates in Montgomery form and canonical (fe381.cuh); Z = 0 is the identity, whatever X and Y
// hold.  a = 0.  The three operations are k_msm.inc's, with its decisions:
//   g1_dbl   2 P for EVERY P (2M + 5S): Z = 0 stays Z = 0 (Z3 = 2 Y Z), and so does Y = 0 (E(Fp) has no such point -- its order is odd -- but the code
//            does not lean on that: the host check doubles one made by hand).
//   g1_add   P + Q for every P, Q (12M + 4S): either at infinity, P = Q (H = 0 and r = 0: the tangent), P = -Q (H = 0 only: the identity).
//   g1_madd  P + (x2, y2) for every Jacobian P and every FINITE affine point (8M + 3S), behind the same decisions.
// The cases are decided on H and r, which are canonical, so "is zero" is exact.
//
// g1_mul: k P for a public 256-bit k and an affine P, left-to-right double-and-add with MIXED additions: 256 doublings and one g1_madd per set bit, about
// 256 * 7 + 128 * 11 = 3 200 field multiplications for a random scalar.  A fixed 4-bit window over the lane's own Jacobian multiples would cost
// 256 * 7 + 64 * 16 + 14 * 16 = 3 040 and needs 15 * 144 bytes of table per lane in memory: 5% fewer multiplications for a table, so there is none.
// The sum is over the integers: P need not lie in G1.  g1_in_subgroup is the definition, [r] P = identity, by the same loop.
#pragma once
#include "fe381.cuh"

namespace ecsimd_hip {

struct g1_point { fe381 x, y, z; };
struct g1_affine { fe381 x, y; };                                     // finite, Montgomery form

// the group order r of G1, 255 bits, as eight words
struct g1_consts { static constexpr uint32_t ORDER[8] = {0x00000001u, 0xffffffffu, 0xfffe5bfeu, 0x53bda402u, 0x09a1d805u, 0x3339d808u, 0x299d7d48u, 0x73eda753u}; };

ECS_HD g1_point g1_identity() { g1_point R; R.x = fe381_zero(); R.y = fe381_zero(); R.z = fe381_zero(); return R; }
ECS_HD bool g1_is_identity(const g1_point& P) { return fe381_is_zero(P.z); }
ECS_HD g1_point g1_from_affine(const g1_affine& a) { g1_point R; R.x = a.x; R.y = a.y; R.z = fe381_one(); return R; }
ECS_HD g1_point g1_neg(const g1_point& P) { g1_point R = P; R.y = fe381_neg(P.y); return R; }
// y^2 = x^3 + 4 for Montgomery-form x, y below p
ECS_HD bool g1_on_curve(const fe381& x, const fe381& y) {
  return fe381_equal(fe381_sqr(y), fe381_add(fe381_mul(fe381_sqr(x), x), fe384_const<bls381_consts::B4>()));
}

ECS_HD g1_point g1_dbl(const g1_point& P) {
  const fe381 YY = fe381_sqr(P.y);
  const fe381 S = fe381_dbl(fe381_dbl(fe381_mul(P.x, YY)));
  const fe381 XX = fe381_sqr(P.x);
  const fe381 M = fe381_add(fe381_dbl(XX), XX);
  g1_point R;
  R.x = fe381_sub(fe381_sqr(M), fe381_dbl(S));
  R.z = fe381_dbl(fe381_mul(P.y, P.z));
  R.y = fe381_sub(fe381_mul(M, fe381_sub(S, R.x)), fe381_dbl(fe381_dbl(fe381_dbl(fe381_sqr(YY)))));
  return R;
}
ECS_HD g1_point g1_add(const g1_point& P, const g1_point& Q) {
  if (fe381_is_zero(P.z)) return Q;
  if (fe381_is_zero(Q.z)) return P;
  const fe381 Z1Z1 = fe381_sqr(P.z), Z2Z2 = fe381_sqr(Q.z);
  const fe381 U1 = fe381_mul(P.x, Z2Z2), U2 = fe381_mul(Q.x, Z1Z1);
  const fe381 S1 = fe381_mul(P.y, fe381_mul(Q.z, Z2Z2)), S2 = fe381_mul(Q.y, fe381_mul(P.z, Z1Z1));
  const fe381 H = fe381_sub(U2, U1), r = fe381_sub(S2, S1);
  if (fe381_is_zero(H)) return fe381_is_zero(r) ? g1_dbl(P) : g1_identity();
  const fe381 HH = fe381_sqr(H), HHH = fe381_mul(H, HH), V = fe381_mul(U1, HH);
  g1_point R;
  R.x = fe381_sub(fe381_sub(fe381_sqr(r), HHH), fe381_dbl(V));
  R.y = fe381_sub(fe381_mul(r, fe381_sub(V, R.x)), fe381_mul(S1, HHH));
  R.z = fe381_mul(fe381_mul(P.z, Q.z), H);
  return R;
}
ECS_HD g1_point g1_madd(const g1_point& P, const fe381& x2, const fe381& y2) {
  if (fe381_is_zero(P.z)) return g1_from_affine({x2, y2});
  const fe381 Z1Z1 = fe381_sqr(P.z);
  const fe381 H = fe381_sub(fe381_mul(x2, Z1Z1), P.x), r = fe381_sub(fe381_mul(y2, fe381_mul(Z1Z1, P.z)), P.y);
  if (fe381_is_zero(H)) return fe381_is_zero(r) ? g1_dbl(g1_from_affine({x2, y2})) : g1_identity();
  const fe381 HH = fe381_sqr(H), HHH = fe381_mul(H, HH), V = fe381_mul(P.x, HH);
  g1_point R;
  R.z = fe381_mul(P.z, H);
  R.x = fe381_sub(fe381_sub(fe381_sqr(r), HHH), fe381_dbl(V));
  R.y = fe381_sub(fe381_mul(r, fe381_sub(V, R.x)), fe381_mul(P.y, HHH));
  return R;
}
// the affine point of a FINITE P: one inversion
ECS_HD g1_affine g1_to_affine(const g1_point& P) {
  const fe381 iz = fe381_invert(P.z), iz2 = fe381_sqr(iz);
  return {fe381_mul(P.x, iz2), fe381_mul(P.y, fe381_mul(iz2, iz))};
}

// k P for the eight little-endian words of a public k (see the head of the file)
ECS_HD g1_point g1_mul(const uint32_t (&k)[8], const g1_affine& P) {
  g1_point acc = g1_identity();
#pragma unroll 1
  for (int w = 7; w >= 0; --w) {
    uint32_t e = 0;
#pragma unroll
    for (int q = 0; q < 8; ++q) e = w == q ? k[q] : e;
#pragma unroll 1
    for (int b = 31; b >= 0; --b) {
      acc = g1_dbl(acc);
      if ((e >> b) & 1u) acc = g1_madd(acc, P.x, P.y);
    }
  }
  return acc;
}
// [r] P is the identity: THE DEFINITION of membership in G1 (the cofactor is 126 bits: most points of E(Fp) fail)
ECS_HD bool g1_in_subgroup(const g1_affine& P) {
  uint32_t k[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) k[q] = g1_consts::ORDER[q];
  return g1_is_identity(g1_mul(k, P));
}

// ---- the serialisation's rules on twelve plain big-endian-decoded words (w[11] holds byte 0 .. 3).  Results: 0 the identity, 1 a point (x, y in Montgomery form), 2 malformed.
constexpr int G1_INFINITY = 0, G1_POINT = 1, G1_MALFORMED = 2;
ECS_HD bool g1_words_zero(const fe381& a, uint32_t top_mask) {
  uint32_t d = a.w[11] & top_mask;
#pragma unroll
  for (int i = 0; i < 11; ++i) d |= a.w[i];
  return d == 0u;
}
// uncompressed: xw, yw as read; flags are the top three bits of xw
ECS_HD int g1_decode96(const fe381& xw, const fe381& yw, g1_affine& out) {
  const uint32_t flags = xw.w[11] >> 29;
  out.x = fe381_zero(); out.y = fe381_zero();
  if (flags == 2u) return (g1_words_zero(xw, 0x1fffffffu) && g1_words_zero(yw, 0xffffffffu)) ? G1_INFINITY : G1_MALFORMED;
  if (flags != 0u || !fe381_below_p(xw) || !fe381_below_p(yw)) return G1_MALFORMED;
  const fe381 x = fe381_to_mont(xw), y = fe381_to_mont(yw);
  if (!g1_on_curve(x, y)) return G1_MALFORMED;
  out.x = x; out.y = y;
  return G1_POINT;
}
// compressed: the x words as read, flags in the top three bits
ECS_HD int g1_decode48(const fe381& cw, g1_affine& out) {
  const uint32_t flags = cw.w[11] >> 29;
  out.x = fe381_zero(); out.y = fe381_zero();
  if (!(flags & 4u)) return G1_MALFORMED;
  if (flags & 2u) return (flags == 6u && g1_words_zero(cw, 0x1fffffffu)) ? G1_INFINITY : G1_MALFORMED;
  fe381 xw = cw; xw.w[11] &= 0x1fffffffu;
  if (!fe381_below_p(xw)) return G1_MALFORMED;
  const fe381 x = fe381_to_mont(xw);
  bool ok;
  fe381 y = fe381_sqrt(fe381_add(fe381_mul(fe381_sqr(x), x), fe384_const<bls381_consts::B4>()), ok);
  if (!ok) return G1_MALFORMED;
  if (fe381_lex_largest(y) != ((flags & 1u) != 0u)) y = fe381_neg(y);
  out.x = x; out.y = y;
  return G1_POINT;
}
// the plain words of the two encodings of a point (cls: G1_INFINITY or G1_POINT)
ECS_HD void g1_encode96(int cls, const g1_affine& a, fe381& xw, fe381& yw) {
  xw = fe381_zero(); yw = fe381_zero();
  if (cls == G1_INFINITY) { xw.w[11] = 0x40000000u; return; }
  xw = fe381_from_mont(a.x); yw = fe381_from_mont(a.y);
}
ECS_HD fe381 g1_encode48(int cls, const g1_affine& a) {
  fe381 cw = fe381_zero();
  if (cls == G1_INFINITY) { cw.w[11] = 0xc0000000u; return cw; }
  cw = fe381_from_mont(a.x);
  cw.w[11] |= 0x80000000u | (fe381_lex_largest(a.y) ? 0x20000000u : 0u);
  return cw;
}

}  // namespace ecsimd_hip
