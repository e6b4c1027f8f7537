// g1.cuh -- the group E(Fp): y^2 = x^3 + 4 of BLS12-381: bls381_curve.inc's law, scalar product, subgroup test and encodings' rules over fe381.cuh, under the
// names g1_*.  This file is the field policy and the inlining policy's default; they stay defined for the including unit (k_bls12_381.inc reads them).  The
// encodings are one 48-byte component per coordinate: 96 bytes, 48 compressed.
#pragma once
#include "fe381.cuh"

namespace ecsimd_hip {
ECS_HD fe381 fe381_curve_b() { return fe384_const<bls381_consts::B4>(); }                           // 4
ECS_HD fe381 fe381_from_wire(const fe381* w) { return fe381_to_mont(w[0]); }
ECS_HD void fe381_to_wire(const fe381& a, fe381* w) { w[0] = fe381_from_mont(a); }
ECS_HD fe381& fe381_component(fe381& a, int) { return a; }                                              // component t of BLS381_COMPONENTS, least significant first
ECS_HD const fe381& fe381_component(const fe381& a, int) { return a; }
}  // namespace ecsimd_hip

#define BLS381_G(name) g1_##name
#define BLS381_F(name) fe381_##name
#define BLS381_ELEM fe381
#define BLS381_COMPONENTS 1
#undef BLS381_MADD_BY_FIELDS
#define BLS381_MADD_BY_FIELDS 1
#ifndef G1_DBL
#define G1_DBL BLS381_INLINE
#endif
#ifndef G1_ADD
#define G1_ADD BLS381_INLINE
#endif
#ifndef G1_MADD
#define G1_MADD BLS381_INLINE
#endif
#define BLS381_DBL_OP G1_DBL
#define BLS381_ADD_OP G1_ADD
#define BLS381_MADD_OP G1_MADD
#include "bls381_curve.inc"

namespace ecsimd_hip {
constexpr int G1_INFINITY = BLS381_INFINITY, G1_POINT = BLS381_POINT, G1_MALFORMED = BLS381_MALFORMED;
// the encodings' rules under their widths' names, on the words of each 48-byte component as read
ECS_HD int g1_decode96(const fe381& xw, const fe381& yw, g1_affine& out) { const fe381 w[2] = {xw, yw}; return g1_decode(w, out); }
ECS_HD int g1_decode48(const fe381& cw, g1_affine& out) { const fe381 w[1] = {cw}; return g1_decode_compressed(w, out); }
ECS_HD void g1_encode96(int cls, const g1_affine& a, fe381& xw, fe381& yw) { fe381 w[2]; g1_encode(cls, a, w); xw = w[0]; yw = w[1]; }
ECS_HD fe381 g1_encode48(int cls, const g1_affine& a) { fe381 w[1]; g1_encode_compressed(cls, a, w); return w[0]; }
}  // namespace ecsimd_hip
