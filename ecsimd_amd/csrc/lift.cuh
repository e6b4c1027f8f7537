// lift.cuh -- from an x coordinate to a curve point: what ECDSA public-key recovery (k_recover.hip) and BIP-340's x-only keys (k_schnorr.hip) share.
// PUBLIC data only: the verdicts are booleans and the callers branch on them.
#pragma once
#include "kernels.h"
#include "point.cuh"
#include "gfield.cuh"

namespace ecsimd_hip {

ECS_DEV fe w8_words(const launch::words8& a) {
  fe r;
#pragma unroll
  for (int k = 0; k < 8; ++k) r.w[k] = a.w[k];
  return r;
}
ECS_DEV fe fe_zero() {
  fe r;
#pragma unroll
  for (int k = 0; k < 8; ++k) r.w[k] = 0;
  return r;
}
// x = r + j n (j = bit 1 of v) as a 256-bit integer; false where v > 3 or the sum does not fit
ECS_DEV bool lift_x(const fe& r, uint32_t v, const launch::words8& order, fe& x) {
  fe add = w8_words(order);
  const uint32_t take = 0u - ((v >> 1) & 1u);
#pragma unroll
  for (int k = 0; k < 8; ++k) add.w[k] &= take;
  x = r;
  const uint32_t carry = add8(x, add);
  return v <= 3u && carry == 0u;
}
// the root with the parity of v's bit 0: y or p - y (false where that is p itself: y = 0 has no odd twin)
ECS_DEV bool pick_parity(fe& y, uint32_t v, const fe& P) {
  fe neg;
  (void)sub8_3(neg, P, y);
  const bool flip = ((y.w[0] ^ v) & 1u) != 0u;
  const bool zero = g_is_zero(y);
  if (flip) y = neg;
  return !(flip && zero);
}
// y = the root of x^3 + a x + b with the parity of v's bit 0, on a built-in curve, in the curve's fast domain (the arithmetic of k_compute_y, k_point.inc);
// false where x >= p, the right-hand side is not a square, or the root of that parity does not exist (y is then not a coordinate)
template <int C> ECS_DEV bool lift_y(const fe& x, uint32_t v, fe& y) {
  constexpr int CI = curve_domain<C>::fast;
  const fe P = FE_CONST(C, P);
  bool ok = g_less(x, P);
  const fe xm = classical_to_fast<C>(x);
  fe rhs = fe_mul<CI>(fe_sqr<CI>(xm), xm);
  if constexpr (curve_prime<C>::is_p256) rhs = fe_sub<CI>(fe_add<CI>(rhs, FE_CONST(CI, BM)), fe_add<CI>(fe_dbl<CI>(xm), xm));   // a = -3
  else rhs = fe_add<CI>(rhs, FE_CONST(CI, BM));                                                                              // a = 0
  const fe root = fe_sqrt_candidate<CI>(rhs);
  ok = ok && fe_eq(fe_sqr<CI>(root), rhs);
  y = fast_to_classical<C>(root);
  return pick_parity(y, v, P) && ok;
}

}  // namespace ecsimd_hip
