// g2.cuh -- the group E'(Fp2): y^2 = x^3 + 4 (1 + u) of BLS12-381: bls381_curve.inc's law, scalar product, subgroup test and encodings' rules over fp2.cuh, under
// the names g2_*.  This file is the field policy and the inlining policy's default; they stay defined for the including unit (k_bls12_381.inc reads them).  The
// encodings are two 48-byte components per coordinate: 192 bytes, 96 compressed.
//
// WIRE ORDER: c1 BEFORE c0 (x.c1 || x.c0 || y.c1 || y.c0), the flag bits in the first byte of x.c1; the lexicographic rule is fp2_lex_largest.
#pragma once
#include "fp2.cuh"

namespace ecsimd_hip {
ECS_HD fp2 fp2_curve_b() { return {fe384_const<bls381_consts::B4>(), fe384_const<bls381_consts::B4>()}; }   // 4 + 4 u
ECS_HD fp2 fp2_from_wire(const fe381* w) { return fp2_to_mont(w[1], w[0]); }
ECS_HD void fp2_to_wire(const fp2& a, fe381* w) { fp2_from_mont(a, w[1], w[0]); }
ECS_HD fe381& fp2_component(fp2& a, int t) { return t == 0 ? a.c0 : a.c1; }                             // component t of BLS381_COMPONENTS, least significant first
ECS_HD const fe381& fp2_component(const fp2& a, int t) { return t == 0 ? a.c0 : a.c1; }
}  // namespace ecsimd_hip

#define BLS381_G(name) g2_##name
#define BLS381_F(name) fp2_##name
#define BLS381_ELEM fp2
#define BLS381_COMPONENTS 2
#undef BLS381_MADD_BY_FIELDS
#define BLS381_MADD_BY_FIELDS 0
#ifndef G2_DBL
#define G2_DBL BLS381_INLINE
#endif
#ifndef G2_ADD
#define G2_ADD BLS381_INLINE
#endif
#ifndef G2_MADD
#define G2_MADD BLS381_INLINE
#endif
#define BLS381_DBL_OP G2_DBL
#define BLS381_ADD_OP G2_ADD
#define BLS381_MADD_OP G2_MADD
#include "bls381_curve.inc"

namespace ecsimd_hip {
constexpr int G2_INFINITY = BLS381_INFINITY, G2_POINT = BLS381_POINT, G2_MALFORMED = BLS381_MALFORMED;
// the encodings' rules under their widths' names, on the words of each 48-byte component as read, in wire order
ECS_HD int g2_decode192(const fe381& x1w, const fe381& x0w, const fe381& y1w, const fe381& y0w, g2_affine& out) { const fe381 w[4] = {x1w, x0w, y1w, y0w}; return g2_decode(w, out); }
ECS_HD int g2_decode96(const fe381& c1w, const fe381& c0w, g2_affine& out) { const fe381 w[2] = {c1w, c0w}; return g2_decode_compressed(w, out); }
ECS_HD void g2_encode192(int cls, const g2_affine& a, fe381& x1w, fe381& x0w, fe381& y1w, fe381& y0w) { fe381 w[4]; g2_encode(cls, a, w); x1w = w[0]; x0w = w[1]; y1w = w[2]; y0w = w[3]; }
ECS_HD void g2_encode96(int cls, const g2_affine& a, fe381& c1w, fe381& c0w) { fe381 w[2]; g2_encode_compressed(cls, a, w); c1w = w[0]; c0w = w[1]; }
}  // namespace ecsimd_hip
