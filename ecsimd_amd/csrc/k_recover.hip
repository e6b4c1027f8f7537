// k_recover.hip -- what ECDSA public-key recovery (SEC 1 v2 4.1.6) and recoverable signing need on top of the existing window loops.
//
// Recovery is Q = u1 G + u2 R with u1 = -e / r, u2 = s / r modulo the group order n and R = (x, y), x = r + j n, y the root of x^3 + a x + b with
// the parity the recovery id asks for: the sum is double_scalar_mult's, the front end is here, two kernels over PUBLIC data:
//   * k_recover_lift<C> / k_gc_recover_lift   modulo p: reads r and v, writes R and a validity byte (v <= 3, x < 2^256, x < p, the right-hand side a
//                                             square, the root of that parity exists); where that fails R = G, a point the sum's window tables can hold;
//   * k_ecdsa_recover_scalars                 modulo n: k_ecdsa_scalars (k_gfield.hip) with the roles of r and s exchanged -- one shared division-step
//                                             inversion of r per up to 128 elements, invalid elements left out of the running product; ANDs the range
//                                             checks 1 <= r, s < n into the validity byte; u1 = u2 = 0 where the element is not valid.
// The order's gmod is a run-time value and the built-in primes are compile-time special forms, hence two kernels; the arrays between them and the sum
// (u1, u2, Rx, Ry, one byte) are written once and read once.
//
// Recoverable signing adds k_sign_recovery_id behind k_ecdsa_sign_scalars: v = parity(y(k G)) | (x(k G) >= n ? 2 : 0), the low-s rule, v = 0 where the
// lane was refused.  The affine k G and the s it may replace are as secret as the nonce until the lane is known to be good: selects only, no branch and no
// address made of them (tools/ct_check.py check_secret_flow holds the ISA to that).
#include "kernels.h"
#include "lift.cuh"
#include "gcurve.cuh"

namespace ecsimd_hip {
namespace {
using launch::BLOCK;
using launch::words8;
#define GID size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x; if (i >= n) return

// built-in curves: lift.cuh's lift_x and lift_y
template <int C> __global__ void __launch_bounds__(BLOCK) k_recover_lift(words8 order, const uint64_t* __restrict__ rv, const uint8_t* __restrict__ vv,
                                                                         uint64_t* __restrict__ ox, uint64_t* __restrict__ oy, uint8_t* __restrict__ valid, size_t n) {
  GID;
  const uint32_t v = vv[i];
  fe x, y;
  bool ok = lift_x(fe_load(rv, i), v, order, x);
  ok = lift_y<C>(x, v, y) && ok;
  if (!ok) { x = FE_CONST(C, GX); y = FE_CONST(C, GY); }
  fe_store(ox, i, x); fe_store(oy, i, y);
  valid[i] = (uint8_t)ok;
}
// a registered curve: the arithmetic of k_gc_compute_y (k_gcurve.hip)
__global__ void __launch_bounds__(BLOCK) k_gc_recover_lift(gcurve G, words8 order, const uint64_t* __restrict__ rv, const uint8_t* __restrict__ vv,
                                                           uint64_t* __restrict__ ox, uint64_t* __restrict__ oy, uint8_t* __restrict__ valid, size_t n) {
  GID;
  const uint32_t v = vv[i];
  const fe P = g_words(G.F.p);
  fe x;
  bool ok = lift_x(fe_load(rv, i), v, order, x);
  ok = ok && g_less(x, P);
  const fe xm = g_from_classical(x, G.F);
  const fe rhs = gc_add(gc_add(gc_mul(gc_sqr<false>(xm, G), xm, G), gc_mul(g_words(G.am), xm, G), G), g_words(G.bm), G);
  const fe root = gc_pow29(rhs, G.F.psqrt, G);
  ok = ok && fe_eq(gc_sqr<false>(root, G), rhs);
  fe y = g_to_classical(root, G.F);
  ok = pick_parity(y, v, P) && ok;
  if (!ok) { x = g_words(G.gx); y = g_words(G.gy); }
  fe_store(ox, i, x); fe_store(oy, i, y);
  valid[i] = (uint8_t)ok;
}

// u1 = -e / r, u2 = s / r modulo n (M = n's gmod), no domain conversion: k_ecdsa_scalars has the algebra (acc_0 = r_0 plain, acc_j = acc_(j-1) r_j / R).
// valid[] comes in as the lift's verdict and leaves as the element's: lift && 1 <= r, s < n.  e is any 256-bit value (g_mul reduces it).
__global__ void __launch_bounds__(256) k_ecdsa_recover_scalars(gmod M, const uint64_t* __restrict__ ev, const uint64_t* __restrict__ rv, const uint64_t* __restrict__ sv,
                                                               uint64_t* __restrict__ u1, uint64_t* __restrict__ u2, uint8_t* __restrict__ valid,
                                                               size_t n, size_t lanes, int m) {
  const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= lanes) return;
  const fe N = g_words(M.p);
  fe one = fe_zero();
  one.w[0] = 1u;
  fe acc = one;
  bool first = true;
  for (int j = 0; j < m; ++j) {
    const size_t e = (size_t)j * lanes + g;
    if (e >= n) break;
    fe r = fe_load(rv, e);
    const fe s = fe_load(sv, e);
    const bool ok = valid[e] != 0 && !g_is_zero(s) && g_less(s, N) && !g_is_zero(r) && g_less(r, N);
    valid[e] = (uint8_t)ok;
    if (!ok) r = one;
    acc = first ? r : g_mul(acc, r, M);
    first = false;
    fe_store(u1, e, acc);
  }
  fe inv = g_inverse_plain(acc, M);
  int last = m - 1;
  while (last >= 0 && (size_t)last * lanes + g >= n) --last;
  const fe rsq = g_words(M.rsq);
  for (int j = last; j >= 0; --j) {
    const size_t e = (size_t)j * lanes + g;
    fe r = fe_load(rv, e);
    const bool ok = valid[e] != 0;
    if (!ok) r = one;
    fe w;
    if (j > 0) { w = g_mul(inv, fe_load(u1, (size_t)(j - 1) * lanes + g), M); inv = g_mul(inv, r, M); }
    else w = inv;
    const fe wr = g_mul(w, rsq, M);                                  // r^-1 R mod n
    fe a = g_sub(fe_zero(), g_mul(fe_load(ev, e), wr, M), M);        // n - e / r (0 stays 0)
    fe b = g_mul(fe_load(sv, e), wr, M);
    if (!ok) { a = fe_zero(); b = fe_zero(); }
    fe_store(u1, e, a);
    fe_store(u2, e, b);
  }
}

// The recovery id of a signature just made, and the low-s rule.  x, y = the affine k G (classical, < p), s = k_ecdsa_sign_scalars' s, ok its verdict.
// Everything a lane computes from x, y and s is data: masks from borrows, selects by masks.  low_s is the call's flag, the same for every lane.
__global__ void __launch_bounds__(BLOCK) k_sign_recovery_id(words8 order, const uint64_t* __restrict__ xv, const uint64_t* __restrict__ yv, uint64_t* __restrict__ sv,
                                                            const uint8_t* __restrict__ okv, uint8_t* __restrict__ vv, size_t n, uint32_t low_s) {
  GID;
  const fe N = w8_words(order);
  fe half;                                                           // n / 2, integer halving
#pragma unroll
  for (int k = 0; k < 7; ++k) half.w[k] = (N.w[k] >> 1) | (N.w[k + 1] << 31);
  half.w[7] = N.w[7] >> 1;
  const fe x = fe_load(xv, i), y = fe_load(yv, i), s = fe_load(sv, i);
  fe d;
  const uint32_t x_below_n = sub8_3(d, x, N);                        // all ones where x < n
  const uint32_t high = sub8_3(d, half, s) & (0u - (low_s & 1u));    // all ones where s > n / 2 and the rule is asked for
  (void)sub8_3(d, N, s);                                             // n - s
  const uint32_t keep = 0u - (uint32_t)(okv[i] != 0);
  uint32_t v = (y.w[0] & 1u) | (~x_below_n & 2u);
  v = (v ^ (high & 1u)) & keep;
  fe_store(sv, i, fe_select(high, d, s));
  vv[i] = (uint8_t)v;
}
}  // namespace

namespace launch {
constexpr size_t RECOVER_BATCH_MAX = 128;          // elements that share one inversion (k_gfield.hip batch_shape)
void ecdsa_recover_scalars(hipStream_t s, const gmod& M, const uint64_t* e, const uint64_t* r, const uint64_t* sg, uint64_t* u1, uint64_t* u2, uint8_t* valid, size_t n) {
  size_t m = n >> 17; if (m < 1) m = 1; if (m > RECOVER_BATCH_MAX) m = RECOVER_BATCH_MAX;
  const size_t lanes = (n + m - 1) / m;
  hipLaunchKernelGGL(k_ecdsa_recover_scalars, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, s, M, e, r, sg, u1, u2, valid, n, lanes, (int)m);
}
void recover_lift(hipStream_t s, int curve, const words8& order, const uint64_t* r, const uint8_t* v, uint64_t* x, uint64_t* y, uint8_t* valid, size_t n) {
  if (curve == CURVE_P256) hipLaunchKernelGGL(k_recover_lift<CURVE_P256>, grid_for(n), dim3(BLOCK), 0, s, order, r, v, x, y, valid, n);
  else hipLaunchKernelGGL(k_recover_lift<CURVE_SECP256K1>, grid_for(n), dim3(BLOCK), 0, s, order, r, v, x, y, valid, n);
}
void gc_recover_lift(hipStream_t s, const gcurve& G, const words8& order, const uint64_t* r, const uint8_t* v, uint64_t* x, uint64_t* y, uint8_t* valid, size_t n) {
  hipLaunchKernelGGL(k_gc_recover_lift, grid_for(n), dim3(BLOCK), 0, s, G, order, r, v, x, y, valid, n);
}
void sign_recovery_id(hipStream_t s, const words8& order, const uint64_t* x, const uint64_t* y, uint64_t* sg, const uint8_t* ok, uint8_t* v, size_t n, bool low_s) {
  hipLaunchKernelGGL(k_sign_recovery_id, grid_for(n), dim3(BLOCK), 0, s, order, x, y, sg, ok, v, n, low_s ? 1u : 0u);
}
}  // namespace launch
}  // namespace ecsimd_hip
