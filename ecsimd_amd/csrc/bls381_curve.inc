// bls381_curve.inc -- y^2 = x^3 + b over a field of BLS12-381, ONCE: the Jacobian group law, the scalar product, the subgroup test and the standard encodings'
// rules.  g1.cuh includes this text for E(Fp), g2.cuh for the twist E'(Fp2); nothing else does.  PUBLIC data only: every exceptional case of the group law, every
// validity test and every scalar bit is a branch.
//
// ONE TEXT, INCLUDED PER GROUP (k_msm.inc's idiom), not templates: DESIGN.md 4n has what the template forms cost in the G1 unit's listing.
//
// THE FIELD POLICY is what the including header defines:
//   BLS381_G(name)        the group's names: g1_##name, g2_##name
//   BLS381_F(name)        the field's functions: fe381_##name, fp2_##name.  Used here: zero one is_zero equal add sub neg dbl mul sqr invert sqrt lex_largest, and
//                         curve_b() (the curve's b), from_wire(w) / to_wire(a, w) between an element and its BLS381_COMPONENTS plain words IN WIRE ORDER: most
//                         significant component first (c1 before c0 for Fp2).
//   BLS381_ELEM           the element type: fe381, fp2
//   BLS381_COMPONENTS     48-byte components of an element: 1, 2.  An encoding is 2 BLS381_COMPONENTS of them, a compressed one BLS381_COMPONENTS.
//   BLS381_MADD_BY_FIELDS how madd takes its affine operand: 1 as its two fields (x2, y2), 0 as ONE reference to the affine point.  It goes with madd's inlining:
//                         inlined into the G1 unit, the single reference costs every kernel around a mixed addition 100 bytes of scratch and k_g1_tree_affine its
//                         third wave per SIMD; out of line in the G2 unit, two fields are three pointers across the call for two and 1% of g2_mul's time
//                         (DESIGN.md 4n).  g1.cuh says 1, g2.cuh 0.
// Elements are canonical Montgomery-form values, so "is zero" and "equal" are exact and the cases below need no normalisation.  Nothing here asks which group it
// serves: what differs comes from these five.  They stay defined after this text, for k_bls12_381.inc; no unit includes both group headers today, and one that
// does must #undef them between the two.
//
// INLINING POLICY: a property the INCLUDING UNIT chooses, per operation, by defining <G>_DBL, <G>_ADD, <G>_MADD (G1_DBL ..., G2_DBL ...) before it includes the
// group's header, each as one of
//   BLS381_INLINE        the operation is inlined into every caller: the default (the G1 unit, the host checks);
//   BLS381_OUT_OF_LINE   ONE copy in the unit, under its own name in the listing, called from everywhere, the nested uses included: add's tangent case and madd's
//                        call dbl, mul's loop calls dbl and madd.
// k_bls12_381_g2.hip chooses out of line for all three (its head says why: an Fp2 product is three Fp products); a unit over a larger field chooses again,
// operation by operation.  The group's header hands the choice on as BLS381_DBL_OP, BLS381_ADD_OP, BLS381_MADD_OP.  Everything else here is always inlined.
//
// Points: Jacobian (X : Y : Z), x = X / Z^2, y = Y / Z^3; Z = 0 is the identity, whatever X and Y hold.  a = 0.  The three operations are k_msm.inc's, with its
// decisions:
//   dbl   2 P for EVERY P (2M + 5S): Z = 0 stays Z = 0 (Z3 = 2 Y Z), and so does Y = 0 (neither curve has such a point -- both orders are odd -- but the code does
//         not lean on that: the host checks double one made by hand).
//   add   P + Q for every P, Q (12M + 4S): either at infinity, P = Q (H = 0 and r = 0: the tangent), P = -Q (H = 0 only: the identity).
//   madd  P + Q for every Jacobian P and every FINITE affine point Q (8M + 3S), behind the same decisions.
// The cases are decided on H and r, which are canonical, so "is zero" is exact.
//
// mul: k P for a public 256-bit k and an affine P, left-to-right double-and-add with MIXED additions: 256 doublings and one madd per set bit, about
// 256 * 7 + 128 * 11 = 3 200 field multiplications for a random scalar.  A fixed 4-bit window over the lane's own Jacobian multiples would cost
// 256 * 7 + 64 * 16 + 14 * 16 = 3 040 and needs 15 * 144 bytes of table per lane in memory (over Fp): 5% fewer multiplications for a table, so there is none.
// The sum is over the integers: P need not lie in the subgroup.  in_subgroup is the definition, [r] P = identity, by the same loop.
#include "fe381.cuh"

#ifndef BLS381_INLINE
#define BLS381_INLINE ECS_HD
#define BLS381_OUT_OF_LINE __host__ __device__ __attribute__((noinline)) static
namespace ecsimd_hip {
// the order r of G1 and of G2, 255 bits, as eight words
struct bls381_order { static constexpr uint32_t WORDS[8] = {0x00000001u, 0xffffffffu, 0xfffe5bfeu, 0x53bda402u, 0x09a1d805u, 0x3339d808u, 0x299d7d48u, 0x73eda753u}; };
// what a decoder says: the identity, a point (x, y in Montgomery form), malformed
constexpr int BLS381_INFINITY = 0, BLS381_POINT = 1, BLS381_MALFORMED = 2;
ECS_HD bool bls381_words_zero(const fe381& a, uint32_t top_mask) {
  uint32_t d = a.w[11] & top_mask;
#pragma unroll
  for (int i = 0; i < 11; ++i) d |= a.w[i];
  return d == 0u;
}
}  // namespace ecsimd_hip
#endif

#define G_ BLS381_G
#define F_ BLS381_F
#define FE BLS381_ELEM
#define NC BLS381_COMPONENTS
// madd's affine operand Q (head of the file): callers write G_(madd)(P, BLS381_Q2(a)) for an affine a, G_(madd)(P, BLS381_Q2_OF(x, y)) for two elements
#if BLS381_MADD_BY_FIELDS
#define Q2_PARAMS const FE& x2, const FE& y2
#define Q2_X x2
#define Q2_Y y2
#define Q2_AFFINE {x2, y2}
#define BLS381_Q2(a) a.x, a.y
#define BLS381_Q2_OF(x, y) x, y
#else
#define Q2_PARAMS const G_(affine)& Q
#define Q2_X Q.x
#define Q2_Y Q.y
#define Q2_AFFINE Q
#define BLS381_Q2(a) a
#define BLS381_Q2_OF(x, y) {x, y}
#endif

namespace ecsimd_hip {

struct G_(point) { FE x, y, z; };
struct G_(affine) { FE x, y; };                                       // finite, Montgomery form

ECS_HD G_(point) G_(identity)() { G_(point) R; R.x = F_(zero)(); R.y = F_(zero)(); R.z = F_(zero)(); return R; }
ECS_HD bool G_(is_identity)(const G_(point)& P) { return F_(is_zero)(P.z); }
ECS_HD G_(point) G_(from_affine)(const G_(affine)& a) { G_(point) R; R.x = a.x; R.y = a.y; R.z = F_(one)(); return R; }
ECS_HD G_(point) G_(neg)(const G_(point)& P) { G_(point) R = P; R.y = F_(neg)(P.y); return R; }
// y^2 = x^3 + b for Montgomery-form x, y
ECS_HD bool G_(on_curve)(const FE& x, const FE& y) { return F_(equal)(F_(sqr)(y), F_(add)(F_(mul)(F_(sqr)(x), x), F_(curve_b)())); }

BLS381_DBL_OP G_(point) G_(dbl)(const G_(point)& P) {
  const FE YY = F_(sqr)(P.y);
  const FE S = F_(dbl)(F_(dbl)(F_(mul)(P.x, YY)));
  const FE XX = F_(sqr)(P.x);
  const FE M = F_(add)(F_(dbl)(XX), XX);
  G_(point) R;
  R.x = F_(sub)(F_(sqr)(M), F_(dbl)(S));
  R.z = F_(dbl)(F_(mul)(P.y, P.z));
  R.y = F_(sub)(F_(mul)(M, F_(sub)(S, R.x)), F_(dbl)(F_(dbl)(F_(dbl)(F_(sqr)(YY)))));
  return R;
}
BLS381_ADD_OP G_(point) G_(add)(const G_(point)& P, const G_(point)& Q) {
  if (F_(is_zero)(P.z)) return Q;
  if (F_(is_zero)(Q.z)) return P;
  const FE Z1Z1 = F_(sqr)(P.z), Z2Z2 = F_(sqr)(Q.z);
  const FE U1 = F_(mul)(P.x, Z2Z2), U2 = F_(mul)(Q.x, Z1Z1);
  const FE S1 = F_(mul)(P.y, F_(mul)(Q.z, Z2Z2)), S2 = F_(mul)(Q.y, F_(mul)(P.z, Z1Z1));
  const FE H = F_(sub)(U2, U1), r = F_(sub)(S2, S1);
  if (F_(is_zero)(H)) return F_(is_zero)(r) ? G_(dbl)(P) : G_(identity)();
  const FE HH = F_(sqr)(H), HHH = F_(mul)(H, HH), V = F_(mul)(U1, HH);
  G_(point) R;
  R.x = F_(sub)(F_(sub)(F_(sqr)(r), HHH), F_(dbl)(V));
  R.y = F_(sub)(F_(mul)(r, F_(sub)(V, R.x)), F_(mul)(S1, HHH));
  R.z = F_(mul)(F_(mul)(P.z, Q.z), H);
  return R;
}
BLS381_MADD_OP G_(point) G_(madd)(const G_(point)& P, Q2_PARAMS) {
  if (F_(is_zero)(P.z)) return G_(from_affine)(Q2_AFFINE);
  const FE Z1Z1 = F_(sqr)(P.z);
  const FE H = F_(sub)(F_(mul)(Q2_X, Z1Z1), P.x), r = F_(sub)(F_(mul)(Q2_Y, F_(mul)(Z1Z1, P.z)), P.y);
  if (F_(is_zero)(H)) return F_(is_zero)(r) ? G_(dbl)(G_(from_affine)(Q2_AFFINE)) : G_(identity)();
  const FE HH = F_(sqr)(H), HHH = F_(mul)(H, HH), V = F_(mul)(P.x, HH);
  G_(point) R;
  R.z = F_(mul)(P.z, H);
  R.x = F_(sub)(F_(sub)(F_(sqr)(r), HHH), F_(dbl)(V));
  R.y = F_(sub)(F_(mul)(r, F_(sub)(V, R.x)), F_(mul)(P.y, HHH));
  return R;
}
// the affine point of a FINITE P: one inversion
ECS_HD G_(affine) G_(to_affine)(const G_(point)& P) {
  const FE iz = F_(invert)(P.z), iz2 = F_(sqr)(iz);
  return {F_(mul)(P.x, iz2), F_(mul)(P.y, F_(mul)(iz2, iz))};
}

// k P for the eight little-endian words of a public k (see the head of the file)
ECS_HD G_(point) G_(mul)(const uint32_t (&k)[8], const G_(affine)& P) {
  G_(point) acc = G_(identity)();
#pragma unroll 1
  for (int w = 7; w >= 0; --w) {
    uint32_t e = 0;
#pragma unroll
    for (int q = 0; q < 8; ++q) e = w == q ? k[q] : e;
#pragma unroll 1
    for (int b = 31; b >= 0; --b) {
      acc = G_(dbl)(acc);
      if ((e >> b) & 1u) acc = G_(madd)(acc, BLS381_Q2(P));
    }
  }
  return acc;
}
// [r] P is the identity: THE DEFINITION of membership in the subgroup (G1's cofactor is 126 bits, G2's 507: most points of either curve fail)
ECS_HD bool G_(in_subgroup)(const G_(affine)& P) {
  uint32_t k[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) k[q] = bls381_order::WORDS[q];
  return G_(is_identity)(G_(mul)(k, P));
}

// ---- the serialisation's rules on plain big-endian-decoded words (w[11] of a component holds its bytes 0 .. 3), components in WIRE order: all of x, then all of
// y, the most significant component of each first, the three flag bits on top of the first (a flag bit in any other component makes it >= p).
// the encodings of the identity: nothing but the flags
template <int N> ECS_HD int G_(decode_infinity)(const fe381 (&w)[N]) {
#pragma unroll
  for (int j = 0; j < N; ++j)
    if (!bls381_words_zero(w[j], j == 0 ? 0x1fffffffu : 0xffffffffu)) return BLS381_MALFORMED;
  return BLS381_INFINITY;
}
// uncompressed: x's components, then y's, as read
ECS_HD int G_(decode)(const fe381 (&w)[2 * NC], G_(affine)& out) {
  const uint32_t flags = w[0].w[11] >> 29;
  out.x = F_(zero)(); out.y = F_(zero)();
  if (flags == 2u) return G_(decode_infinity)(w);
  if (flags != 0u) return BLS381_MALFORMED;
#pragma unroll
  for (int j = 0; j < 2 * NC; ++j)
    if (!fe381_below_p(w[j])) return BLS381_MALFORMED;
  const FE x = F_(from_wire)(w), y = F_(from_wire)(w + NC);
  if (!G_(on_curve)(x, y)) return BLS381_MALFORMED;
  out.x = x; out.y = y;
  return BLS381_POINT;
}
// compressed: x's components as read
ECS_HD int G_(decode_compressed)(const fe381 (&w)[NC], G_(affine)& out) {
  const uint32_t flags = w[0].w[11] >> 29;
  out.x = F_(zero)(); out.y = F_(zero)();
  if (!(flags & 4u)) return BLS381_MALFORMED;
  if (flags & 2u) return flags == 6u ? G_(decode_infinity)(w) : BLS381_MALFORMED;
  fe381 xw[NC];
#pragma unroll
  for (int j = 0; j < NC; ++j) xw[j] = w[j];
  xw[0].w[11] &= 0x1fffffffu;
#pragma unroll
  for (int j = 0; j < NC; ++j)
    if (!fe381_below_p(xw[j])) return BLS381_MALFORMED;
  const FE x = F_(from_wire)(xw);
  bool ok;
  FE y = F_(sqrt)(F_(add)(F_(mul)(F_(sqr)(x), x), F_(curve_b)()), ok);
  if (!ok) return BLS381_MALFORMED;
  if (F_(lex_largest)(y) != ((flags & 1u) != 0u)) y = F_(neg)(y);
  out.x = x; out.y = y;
  return BLS381_POINT;
}
// the plain words of the two encodings of a point (cls: BLS381_INFINITY or BLS381_POINT), in wire order; the compressed one of BLS381_MALFORMED is all zero
ECS_HD void G_(encode)(int cls, const G_(affine)& a, fe381 (&w)[2 * NC]) {
#pragma unroll
  for (int j = 0; j < 2 * NC; ++j) w[j] = fe381_zero();
  if (cls == BLS381_INFINITY) { w[0].w[11] = 0x40000000u; return; }
  F_(to_wire)(a.x, w); F_(to_wire)(a.y, w + NC);
}
ECS_HD void G_(encode_compressed)(int cls, const G_(affine)& a, fe381 (&w)[NC]) {
#pragma unroll
  for (int j = 0; j < NC; ++j) w[j] = fe381_zero();
  if (cls == BLS381_MALFORMED) return;
  if (cls == BLS381_INFINITY) { w[0].w[11] = 0xc0000000u; return; }
  F_(to_wire)(a.x, w);
  w[0].w[11] |= 0x80000000u | (F_(lex_largest)(a.y) ? 0x20000000u : 0u);
}

}  // namespace ecsimd_hip

#undef G_
#undef F_
#undef FE
#undef NC
#undef Q2_PARAMS
#undef Q2_X
#undef Q2_Y
#undef Q2_AFFINE
