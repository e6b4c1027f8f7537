// k_msm.inc -- multi-scalar multiplication R = sum k_i P_i and the point sum over lanes, for ONE curve (included with ECS_CURVE defined): the kernels behind
// ecsimd_msm / ecsimd_msm_point_sum (include/ecsimd_msm.h).  PUBLIC data only: bucket addresses are scalar digits and every exceptional case of the group law
// is a branch.  The schedule -- which kernels, how many lanes, how long a lane's loop -- is a function of (n, bits, flags) alone (capi.hip msm_schedule_of,
// tools/msm_model.py); the data decide only which side of a branch a lane takes.
//
// The BUCKETS route: msm_stages.cuh has the stages and their bodies; this file gives them the Jacobian group (complete additions: every exceptional case of the
// group law decided by a branch) and keeps what is the curve's: k_msm_digits validates the point as k_on_curve validates and converts it to the fast domain,
// k_msm_final ends Horner with ONE inversion, the affine classical result, the flag and the invalid count.  k_msm_common.hip has zero, scan and scatter.
// The LANES route: k_msm_sanitize (the same validation; (0, G) where a term contributes nothing), the per-lane windowed products of k_varwin.inc, then
// k_msm_tree_affine / k_msm_tree / k_msm_final.  ecsimd_msm_point_sum is k_msm_tree_affine with the validation on, then the same two.
//
// Arithmetic: field.cuh's canonical words (as madd_hmv); Jacobian coordinates in the fast domain, Z = 0 is infinity.  Jacobian arrays are three planes of
// `total` elements: x at e, y at total + e, z at 2 total + e.
// Registers and scratch (build/csrc/k_msm_<curve>-hip-amdgcn-amd-amdhsa-gfx950.s; profiles/r15/msm_listing.json and DESIGN.md have the table): no kernel spills.
// 256-thread workgroups throughout.  Of the 512 VGPRs a SIMD gives a lane, the kernels around one mixed addition (slices, tree_affine, the last) take 106 - 124:
// 4 waves per SIMD; those with two Jacobian operands or more live across a general addition (combine, tree, chunks: run, tot and the multiple) take 124 - 184:
// 3 waves, 2 for k_msm_chunks on secp256k1.  The 68 bytes of scratch of k_msm_slices and k_msm_tree_affine are below what the other public-data kernels with
// a loop around an addition use (112 - 768).
#include "kernels.h"
#include "point.cuh"
#include "msm_stages.cuh"

namespace ecsimd_hip {
namespace {
constexpr int C = ECS_CURVE;
constexpr int CI = curve_domain<C>::fast;
using launch::BLOCK;

ECS_DEV bool fe_is_zero(const fe& a) {
  uint32_t d = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) d |= a.w[i];
  return d == 0;
}
ECS_DEV fe fe_zero() {
  fe r;
#pragma unroll
  for (int i = 0; i < 8; ++i) r.w[i] = 0;
  return r;
}
ECS_DEV bool below_p(const fe& v) {
  fe t = v; const fe p = FE_CONST(C, P);
  return sub8(t, p) != 0u;                                              // borrow <=> v < p
}
ECS_DEV jpoint j_infinity() { jpoint R; R.x = fe_zero(); R.y = fe_zero(); R.z = fe_zero(); return R; }
ECS_DEV jpoint j_load(const uint64_t* __restrict__ a, size_t total, size_t e) {
  jpoint R; R.x = fe_load(a, e); R.y = fe_load(a, total + e); R.z = fe_load(a, 2 * total + e); return R;
}
ECS_DEV void j_store(uint64_t* __restrict__ a, size_t total, size_t e, const jpoint& P) {
  fe_store(a, e, P.x); fe_store(a, total + e, P.y); fe_store(a, 2 * total + e, P.z);
}

// 2 P for every P: Z = 0 stays Z = 0 (Z3 = 2 Y Z), and so does Y = 0.  a = -3: M = 3 (X - Z^2)(X + Z^2); a = 0: M = 3 X^2.
ECS_DEV jpoint j_dbl(const jpoint& P) {
  const fe YY = fe_sqr<CI>(P.y);
  const fe S = fe_shl<CI, 2>(fe_mul<CI>(P.x, YY));
  fe M;
  if constexpr (curve_prime<C>::is_p256) {
    const fe ZZ = fe_sqr<CI>(P.z);
    const fe t = fe_mul<CI>(fe_sub<CI>(P.x, ZZ), fe_add<CI>(P.x, ZZ));
    M = fe_add<CI>(fe_dbl<CI>(t), t);
  } else {
    const fe XX = fe_sqr<CI>(P.x);
    M = fe_add<CI>(fe_dbl<CI>(XX), XX);
  }
  jpoint R;
  R.x = fe_sub<CI>(fe_sqr<CI>(M), fe_dbl<CI>(S));
  R.z = fe_dbl<CI>(fe_mul<CI>(P.y, P.z));
  R.y = fe_sub<CI>(fe_mul<CI>(M, fe_sub<CI>(S, R.x)), fe_shl<CI, 3>(fe_sqr<CI>(YY)));
  return R;
}
// P + Q for every P, Q (12M + 4S): either at infinity, P = Q (the tangent), P = -Q (infinity).  The cases are decided on H and r, not assumed away.
ECS_DEV jpoint j_add(const jpoint& P, const jpoint& Q) {
  if (fe_is_zero(P.z)) return Q;
  if (fe_is_zero(Q.z)) return P;
  const fe Z1Z1 = fe_sqr<CI>(P.z), Z2Z2 = fe_sqr<CI>(Q.z);
  const fe U1 = fe_mul<CI>(P.x, Z2Z2), U2 = fe_mul<CI>(Q.x, Z1Z1);
  const fe S1 = fe_mul<CI>(P.y, fe_mul<CI>(Q.z, Z2Z2)), S2 = fe_mul<CI>(Q.y, fe_mul<CI>(P.z, Z1Z1));
  const fe H = fe_sub<CI>(U2, U1), r = fe_sub<CI>(S2, S1);
  if (fe_is_zero(H)) return fe_is_zero(r) ? j_dbl(P) : j_infinity();
  const fe HH = fe_sqr<CI>(H), HHH = fe_mul<CI>(H, HH), V = fe_mul<CI>(U1, HH);
  jpoint R;
  R.x = fe_sub<CI>(fe_sub<CI>(fe_sqr<CI>(r), HHH), fe_dbl<CI>(V));
  R.y = fe_sub<CI>(fe_mul<CI>(r, fe_sub<CI>(V, R.x)), fe_mul<CI>(S1, HHH));
  R.z = fe_mul<CI>(fe_mul<CI>(P.z, Q.z), H);
  return R;
}
// P + (x2, y2) for every Jacobian P and every FINITE affine point of the curve (fast domain): madd_hmv's formulas (8M + 3S) behind the same decisions.
ECS_DEV jpoint j_madd(const jpoint& P, const fe& x2, const fe& y2) {
  jpoint A; A.x = x2; A.y = y2; A.z = FE_CONST(CI, R_P);
  if (fe_is_zero(P.z)) return A;
  const fe Z1Z1 = fe_sqr<CI>(P.z);
  const fe H = fe_sub<CI>(fe_mul<CI>(x2, Z1Z1), P.x), r = fe_sub<CI>(fe_mul<CI>(y2, fe_mul<CI>(Z1Z1, P.z)), P.y);
  if (fe_is_zero(H)) return fe_is_zero(r) ? j_dbl(A) : j_infinity();
  const fe HH = fe_sqr<CI>(H), HHH = fe_mul<CI>(H, HH), V = fe_mul<CI>(P.x, HH);
  jpoint R;
  R.z = fe_mul<CI>(P.z, H);
  R.x = fe_sub<CI>(fe_sub<CI>(fe_sqr<CI>(r), HHH), fe_dbl<CI>(V));
  R.y = fe_sub<CI>(fe_mul<CI>(r, fe_sub<CI>(V, R.x)), fe_mul<CI>(P.y, HHH));
  return R;
}

// 0 the point at infinity (0, 0): contributes nothing and is not an error; 1 a point of the curve (xf, yf = its fast-domain coordinates); 2 invalid.
ECS_DEV int classify(const fe& xv, const fe& yv, fe& xf, fe& yf) {
  if (fe_is_zero(xv) && fe_is_zero(yv)) return 0;
  xf = classical_to_fast<C>(xv); yf = classical_to_fast<C>(yv);
  fe rhs = fe_mul<CI>(fe_sqr<CI>(xf), xf);
  if constexpr (curve_prime<C>::is_p256) rhs = fe_sub<CI>(fe_add<CI>(rhs, FE_CONST(CI, BM)), fe_add<CI>(fe_dbl<CI>(xf), xf));
  else rhs = fe_add<CI>(rhs, FE_CONST(CI, BM));
  return (below_p(xv) && below_p(yv) && fe_eq(fe_sqr<CI>(yf), rhs)) ? 1 : 2;
}
// msm_stages.cuh's group: Jacobian accumulators, three planes, Z = 0; the terms are the affine fast-domain points k_msm_digits left at (px, py)
struct jacobian_group {
  using point = jpoint;
  struct terms { const uint64_t* __restrict__ px; const uint64_t* __restrict__ py; };
  ECS_DEV static point identity() { return j_infinity(); }
  ECS_DEV static point add(const point& P, const point& Q) { return j_add(P, Q); }
  ECS_DEV static point dbl(const point& P) { return j_dbl(P); }
  ECS_DEV static point add_term(const point& P, const terms& t, size_t, size_t idx) { return j_madd(P, fe_load(t.px, idx), fe_load(t.py, idx)); }
  ECS_DEV static point load(const uint64_t* __restrict__ a, size_t total, size_t e) { return j_load(a, total, e); }
  ECS_DEV static void store(uint64_t* __restrict__ a, size_t total, size_t e, const point& P) { j_store(a, total, e, P); }
};
using G = jacobian_group;

__global__ void __launch_bounds__(BLOCK) k_msm_digits(const uint64_t* __restrict__ k, const uint64_t* __restrict__ x, const uint64_t* __restrict__ y, uint64_t* __restrict__ kk,
                                                      uint64_t* __restrict__ px, uint64_t* __restrict__ py, uint32_t* __restrict__ hist, uint32_t* __restrict__ counter,
                                                      size_t n, int bits, int c, int windows) {
  const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n) return;
  fe xf = fe_zero(), yf = fe_zero();
  const int cls = classify(fe_load(x, i), fe_load(y, i), xf, yf);
  if (cls == 2) atomicAdd(counter, 1u);
  const fe kv = cls == 1 ? mask_bits(fe_load(k, i), bits) : fe_zero();
  fe_store(kk, i, kv); fe_store(px, i, xf); fe_store(py, i, yf);
  msm_histogram(kv, hist, c, windows);
}

__global__ void __launch_bounds__(BLOCK) k_msm_slices(const uint32_t* __restrict__ sorted, const uint64_t* __restrict__ kk, const uint64_t* __restrict__ px,
                                                      const uint64_t* __restrict__ py, const uint32_t* __restrict__ start, uint64_t* __restrict__ buckets,
                                                      uint64_t* __restrict__ partial, uint32_t* __restrict__ broken, size_t n, size_t T, size_t L, size_t slices, int c, size_t K) {
  msm_slices<G>(sorted, kk, {px, py}, start, buckets, partial, broken, n, T, L, slices, c, K);
}
__global__ void __launch_bounds__(BLOCK) k_msm_combine(const uint32_t* __restrict__ start, uint64_t* __restrict__ buckets, const uint64_t* __restrict__ partial,
                                                       uint32_t* __restrict__ broken, size_t L, size_t slices, int c, size_t K) {
  msm_combine<G>(start, buckets, partial, broken, L, slices, c, K);
}
__global__ void __launch_bounds__(BLOCK) k_msm_chunks(const uint64_t* __restrict__ buckets, uint64_t* __restrict__ out, size_t lanes, size_t per_window, int c, int m, size_t K) {
  msm_chunks<G>(buckets, out, lanes, per_window, c, m, K);
}
__global__ void __launch_bounds__(BLOCK) k_msm_tree(uint64_t* arr, size_t total, size_t count, size_t stride, size_t lanes, int fan) {
  msm_tree<G>(arr, total, count, stride, lanes, fan);
}
// the same from affine classical points ((0, 0) = infinity) into a Jacobian array; VALIDATE: each point checked as k_msm_digits checks it, invalid ones counted and skipped
template <bool VALIDATE>
__global__ void __launch_bounds__(BLOCK) k_msm_tree_affine(const uint64_t* __restrict__ x, const uint64_t* __restrict__ y, uint32_t* __restrict__ counter, uint64_t* __restrict__ out,
                                                           size_t n, size_t lanes, int fan) {
  const size_t g = (size_t)blockIdx.x * BLOCK + threadIdx.x;
  if (g >= lanes) return;
  jpoint acc = j_infinity();
#pragma unroll 1
  for (int t = 0; t < fan; ++t) {
    const size_t e = g + (size_t)t * lanes;
    if (e >= n) break;
    const fe xv = fe_load(x, e), yv = fe_load(y, e);
    fe xf, yf;
    if constexpr (VALIDATE) {
      const int cls = classify(xv, yv, xf, yf);
      if (cls == 2) atomicAdd(counter, 1u);
      if (cls != 1) continue;
    } else {
      if (fe_is_zero(xv) && fe_is_zero(yv)) continue;
      xf = classical_to_fast<C>(xv); yf = classical_to_fast<C>(yv);
    }
    acc = j_madd(acc, xf, yf);
  }
  j_store(out, lanes, g, acc);
}

// The LANES route's front: the masked scalar and the point as the per-lane product takes them; a term that contributes nothing becomes 0 * G.
__global__ void __launch_bounds__(BLOCK) k_msm_sanitize(const uint64_t* __restrict__ k, const uint64_t* __restrict__ x, const uint64_t* __restrict__ y, uint64_t* __restrict__ kk,
                                                        uint64_t* __restrict__ sx, uint64_t* __restrict__ sy, uint32_t* __restrict__ counter, size_t n, int bits) {
  const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n) return;
  fe xv = fe_load(x, i), yv = fe_load(y, i), xf, yf;
  const int cls = classify(xv, yv, xf, yf);
  if (cls == 2) atomicAdd(counter, 1u);
  fe kv = mask_bits(fe_load(k, i), bits);
  if (cls != 1) { kv = fe_zero(); xv = FE_CONST(C, GX); yv = FE_CONST(C, GY); }
  fe_store(kk, i, kv); fe_store(sx, i, xv); fe_store(sy, i, yv);
}

// One lane: msm_horner, then the affine classical result.
__global__ void __launch_bounds__(64) k_msm_final(const uint64_t* __restrict__ arr, size_t total, size_t stride, int windows, int c, const uint32_t* __restrict__ counter,
                                                  uint64_t* __restrict__ rx, uint64_t* __restrict__ ry, uint8_t* __restrict__ finite, uint32_t* __restrict__ invalid) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const jpoint acc = msm_horner<G>(arr, total, stride, windows, c);
  fe ax = fe_zero(), ay = fe_zero();
  const bool fin = !fe_is_zero(acc.z);
  if (fin) {
    const fe iz = fe_inverse<CI>(acc.z), iz2 = fe_sqr<CI>(iz);
    ax = fast_to_classical<C>(fe_mul<CI>(acc.x, iz2));
    ay = fast_to_classical<C>(fe_mul<CI>(acc.y, fe_mul<CI>(iz2, iz)));
  }
  uint32_t bad = counter ? counter[0] : 0u;
  if (counter && counter[1] != 0u) {                                    // a broken invariant of the sort: no sum is better than a wrong one (ecsimd_msm.h, INTERNAL CHECK)
#pragma unroll
    for (int j = 0; j < 8; ++j) { ax.w[j] = 0xffffffffu; ay.w[j] = 0xffffffffu; }
    bad = 0xffffffffu;
  }
  fe_store(rx, 0, ax); fe_store(ry, 0, ay);
  finite[0] = (uint8_t)((fin || bad == 0xffffffffu) ? 1 : 0);
  if (invalid) invalid[0] = bad;
}
}  // namespace

namespace launch {
static dim3 grid_of(size_t lanes, size_t y = 1) { return dim3((unsigned)((lanes + BLOCK - 1) / BLOCK), (unsigned)y); }
template <> void msm_launch<C>::digits(hipStream_t s, const uint64_t* k, const uint64_t* x, const uint64_t* y, uint64_t* kk, uint64_t* px, uint64_t* py, uint32_t* hist,
                                       uint32_t* counter, size_t n, int bits, int c, int windows) {
  hipLaunchKernelGGL(k_msm_digits, grid_of(n), dim3(BLOCK), 0, s, k, x, y, kk, px, py, hist, counter, n, bits, c, windows);
}
template <> void msm_launch<C>::slices(hipStream_t s, const uint32_t* sorted, const uint64_t* kk, const uint64_t* px, const uint64_t* py, const uint32_t* start, uint64_t* buckets,
                                       uint64_t* partial, uint32_t* broken, size_t n, size_t T, size_t L, size_t slices, int c, size_t K) {
  hipLaunchKernelGGL(k_msm_slices, grid_of(slices), dim3(BLOCK), 0, s, sorted, kk, px, py, start, buckets, partial, broken, n, T, L, slices, c, K);
}
template <> void msm_launch<C>::combine(hipStream_t s, const uint32_t* start, uint64_t* buckets, const uint64_t* partial, uint32_t* broken, size_t L, size_t slices, int c, size_t K) {
  hipLaunchKernelGGL(k_msm_combine, grid_of(K), dim3(BLOCK), 0, s, start, buckets, partial, broken, L, slices, c, K);
}
template <> void msm_launch<C>::chunks(hipStream_t s, const uint64_t* buckets, uint64_t* out, size_t lanes, size_t per_window, int c, int m, size_t K) {
  hipLaunchKernelGGL(k_msm_chunks, grid_of(lanes), dim3(BLOCK), 0, s, buckets, out, lanes, per_window, c, m, K);
}
template <> void msm_launch<C>::tree(hipStream_t s, uint64_t* arr, size_t total, size_t count, size_t stride, size_t groups, size_t lanes, int fan) {
  hipLaunchKernelGGL(k_msm_tree, grid_of(lanes, groups), dim3(BLOCK), 0, s, arr, total, count, stride, lanes, fan);
}
template <> void msm_launch<C>::tree_affine(hipStream_t s, const uint64_t* x, const uint64_t* y, bool validate, uint32_t* counter, uint64_t* out, size_t n, size_t lanes, int fan) {
  if (validate) hipLaunchKernelGGL(k_msm_tree_affine<true>, grid_of(lanes), dim3(BLOCK), 0, s, x, y, counter, out, n, lanes, fan);
  else hipLaunchKernelGGL(k_msm_tree_affine<false>, grid_of(lanes), dim3(BLOCK), 0, s, x, y, counter, out, n, lanes, fan);
}
template <> void msm_launch<C>::sanitize(hipStream_t s, const uint64_t* k, const uint64_t* x, const uint64_t* y, uint64_t* kk, uint64_t* sx, uint64_t* sy, uint32_t* counter,
                                         size_t n, int bits) {
  hipLaunchKernelGGL(k_msm_sanitize, grid_of(n), dim3(BLOCK), 0, s, k, x, y, kk, sx, sy, counter, n, bits);
}
template <> void msm_launch<C>::finish(hipStream_t s, const uint64_t* arr, size_t total, size_t stride, int windows, int c, const uint32_t* counter, uint64_t* rx, uint64_t* ry,
                                      uint8_t* finite, uint32_t* invalid) {
  hipLaunchKernelGGL(k_msm_final, dim3(1), dim3(64), 0, s, arr, total, stride, windows, c, counter, rx, ry, finite, invalid);
}
}  // namespace launch
}  // namespace ecsimd_hip
