// k_ladder.inc -- the scalar-multiplication kernel for ONE curve (curve_group.h:189-251,
// lib/scalar_mult_p256.cpp:10-12).  Included with ECS_CURVE defined.
//
// One kernel serves scalar_mult, scalar_mult_1s (k_stride = 0: every lane reads the same scalar
// words, a broadcast load), scalar_mult_base (x == nullptr: generator) and both input/output
// forms; the options are wave-uniform branches outside the 254-iteration ZDAU loop.  With
// OUT_AFFINE the kernel writes the Jacobian result in the fast domain into (ox, oy, oz) = scratch.
#include "kernels.h"
#include "point.cuh"
#include "../../include/ecsimd_hip.h"

namespace ecsimd_hip {
namespace {
using launch::BLOCK;
constexpr int C = ECS_CURVE;
#ifndef LADDER_WAVES_PER_SIMD
#define LADDER_WAVES_PER_SIMD 3   // 168 VGPRs at most.  P-256 allocates 147; secp256k1, with ZDAU's Z update placed early (point.cuh
                                  // zdau_z_early), 162 and no spill -- before round 3 it hit the cap with 14 registers spilled (all but the
                                  // scalar pointer's reload outside the bit loop: 48.41 against 48.33 M/s, nothing to gain either way)
#endif

// RADIX: the representation the 254-iteration loop runs in -- 32: field.cuh's canonical 8 x 32-bit words (rounds 1-3, what the
// reference-square instances need, and ECSIMD_HIP_LADDER_RADIX32); 29: fe29.cuh's nine signed 29-bit limbs (round 4; the default where
// it exists).  Same results.
constexpr bool HAS_R29 = ladder_has_radix29<curve_domain<C>::fast>::value;
template <int RADIX> __global__ void __launch_bounds__(BLOCK, LADDER_WAVES_PER_SIMD)
k_scalar_mult(const uint64_t* __restrict__ k, int k_stride, const uint64_t* __restrict__ x, const uint64_t* __restrict__ y,
              uint64_t* __restrict__ ox, uint64_t* __restrict__ oy, uint64_t* __restrict__ oz, size_t n, int flags) {
  const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n) return;
  // CI = the domain the ladder runs in: Montgomery for P-256, classical for secp256k1 (field.cuh).
  constexpr int CI = curve_domain<C>::fast;
  fe xm, ym;
  if (x == nullptr) { xm = FE_CONST(C, GX); ym = FE_CONST(C, GY); }          // classical constants
  else { xm = fe_load(x, i); ym = fe_load(y, i); }
  const bool in_mgry = (x != nullptr) && (flags & ECSIMD_HIP_BASE_MGRY);
  if constexpr (CI == C) { if (!in_mgry) { xm = fe_from_classical<C>(xm); ym = fe_from_classical<C>(ym); } }
  else { if (in_mgry) { xm = fe_to_classical<C>(xm); ym = fe_to_classical<C>(ym); } }
  const uint32_t* kw = reinterpret_cast<const uint32_t*>(k + (size_t)k_stride * i);
  const jpoint R = scalar_mult_ladder<CI, RADIX>(kw, xm, ym);
  // OUT_AFFINE: the launcher follows up with the simultaneous-inversion kernel (k_affine.inc), which
  // takes the point in the fast domain -- so the Jacobian result is stored as is.  Keeping the 267-mult
  // per-lane inversion out of this kernel also keeps its register allocation at the ZDAU loop's.
  if ((flags & ECSIMD_HIP_OUT_AFFINE) || CI == C) {
    fe_store(ox, i, R.x); fe_store(oy, i, R.y); fe_store(oz, i, R.z);
  } else {
    fe_store(ox, i, fe_from_classical<C>(R.x)); fe_store(oy, i, fe_from_classical<C>(R.y)); fe_store(oz, i, fe_from_classical<C>(R.z));
  }
}

// The loop body alone, `iters` times in registers (ecsimd_hip_zdau_repeat): (P, Q) <- (2P + Q, Q re-expressed), the two outputs exchanged
// after iteration t where bit (t mod 64) of swap_bits is set -- the ladder's loop with a public swap pattern.  In and out: the API's
// Montgomery form.  The micro-kernel behind profiles/r04/zdau_radix.txt and the parity test of the reduced-radix ZDAU.
template <int RADIX> __global__ void __launch_bounds__(BLOCK, LADDER_WAVES_PER_SIMD)
k_zdau_repeat(const uint64_t* __restrict__ px, const uint64_t* __restrict__ py, const uint64_t* __restrict__ pz, const uint64_t* __restrict__ qx, const uint64_t* __restrict__ qy,
              uint64_t* __restrict__ rx, uint64_t* __restrict__ ry, uint64_t* __restrict__ sx, uint64_t* __restrict__ sy, uint64_t* __restrict__ oz, size_t n, int iters, uint64_t swap_bits) {
  const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n) return;
  constexpr int CI = curve_domain<C>::fast;
  fe x1 = to_fast<C>(fe_load(px, i)), y1 = to_fast<C>(fe_load(py, i)), z = to_fast<C>(fe_load(pz, i)), x2 = to_fast<C>(fe_load(qx, i)), y2 = to_fast<C>(fe_load(qy, i));
  if constexpr (RADIX == 29) {
    coz29 s;
    s.x1 = enter29<CI>(x1); s.x2 = enter29<CI>(x2); s.y1 = enter29<CI>(y1); s.z = enter29<CI>(z);
    s.dx = sub29(s.x1, s.x2);
    s.dy = sub29(s.y1, enter29<CI>(y2));
#pragma unroll 1
    for (int t = 0; t < iters; ++t) zdau29<CI>(s, 0u - (uint32_t)((swap_bits >> (t & 63)) & 1u));
    x1 = leave29<CI>(s.x1); y1 = leave29<CI>(s.y1); x2 = leave29<CI>(s.x2); y2 = leave29<CI>(sub29(s.y1, s.dy)); z = leave29<CI>(s.z);
  } else {
    // The loop state must not live in the 128-bit register tuples of the loads / stores: with z.w[4..7] loop-carried as lanes of such a
    // tuple the compiler merged mac_col's early-clobber carry counter into the lane of the still-live z.w[7] (a wrong Z on the GPU; every
    // perturbation of the formulas kept the defect).  One v_mov per word on the way in and out gives the loop plain 32-bit registers,
    // as the ladder kernel has them (its state comes out of asm statements).  tools/asm_clobber_check.py, tests/test_isa_guards.py.
    auto fresh = [](fe& v) {
#pragma unroll
      for (int w = 0; w < 8; ++w) asm volatile("v_mov_b32 %0, %1" : "=v"(v.w[w]) : "v"(v.w[w]));
    };
    fresh(x1); fresh(y1); fresh(x2); fresh(y2); fresh(z);
#pragma unroll 1
    for (int t = 0; t < iters; ++t) zdau<CI>(x1, y1, x2, y2, z, 0u - (uint32_t)((swap_bits >> (t & 63)) & 1u));
    fresh(x1); fresh(y1); fresh(x2); fresh(y2); fresh(z);
  }
  fe_store(rx, i, from_fast<C>(x1)); fe_store(ry, i, from_fast<C>(y1)); fe_store(sx, i, from_fast<C>(x2)); fe_store(sy, i, from_fast<C>(y2)); fe_store(oz, i, from_fast<C>(z));
}

#ifdef ECS_LADDER_X
// ---------------------------------------------------------------- x-coordinate only (ECDH's shared secret)
// x(kP) = x((n - k)P), and of k mod n and n - (k mod n) exactly one is odd (n is odd): the ladder runs on that one, which
// needs no even-k correction -- the one step of the reference's ladder that cannot do without Z (and its sign).
// state[j]: 1 = (k = 0 mod n): the product is the point at infinity, x := 0 like to_affine's.
//           2 = k mod n is 2^256 mod n or its negative: for the odd one of the two, c = 2^256 - n, the ladder's other
//               register ends at (2^256 - c)P = nP = infinity and takes the co-Z pair with it (it is one of the reference
//               ladder's own degenerate scalars), and no other odd 256-bit integer is congruent to +-c.  Those lanes get
//               the even n - c and are redone by k_x_fixup with the reference's full ladder, which is sound there.
__global__ void __launch_bounds__(BLOCK) k_odd_scalar(const uint64_t* __restrict__ k, uint64_t* __restrict__ kodd, uint8_t* __restrict__ state, size_t m) {
  const size_t j = (size_t)blockIdx.x * BLOCK + threadIdx.x;
  if (j >= m) return;
  const fe v = fe_load(k, j);
  fe order, zero, d, neg, c, nc;
#pragma unroll
  for (int w = 0; w < 8; ++w) { order.w[w] = curve_order<C>::N[w]; zero.w[w] = 0; }
  const uint32_t below = sub8_3(d, v, order);              // k < 2^256 < 2n: one conditional subtraction reduces k
  const fe kr = fe_select(below, v, d);
  (void)sub8_3(neg, order, kr);                            // n - kr  (= n for kr = 0: flagged)
  (void)sub8_3(c, zero, order);                            // 2^256 - n
  (void)sub8_3(nc, order, c);
  uint32_t any = 0;
#pragma unroll
  for (int w = 0; w < 8; ++w) any |= kr.w[w];
  const bool special = (int)fe_eq(kr, c) | (int)fe_eq(kr, nc);          // both compared: no branch on the scalar
  const uint32_t odd = 0u - (kr.w[0] & 1u);
  fe_store(kodd, j, special ? nc : fe_select(odd, kr, neg));
  state[j] = (uint8_t)(any == 0 ? 1 : special ? 2 : 0);
}
__global__ void __launch_bounds__(BLOCK, LADDER_WAVES_PER_SIMD)
k_scalar_mult_x(const uint64_t* __restrict__ kodd, int k_stride, const uint64_t* __restrict__ x, const uint64_t* __restrict__ y,
                uint64_t* __restrict__ num, uint64_t* __restrict__ den, size_t n, int flags) {
  const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n) return;
  static_assert(curve_domain<C>::fast == C, "the x-only ladder runs in the API's Montgomery domain");
  fe xm, ym;
  if (x == nullptr) { xm = fe_from_classical<C>(FE_CONST(C, GX)); ym = fe_from_classical<C>(FE_CONST(C, GY)); }
  else {
    xm = fe_load(x, i); ym = fe_load(y, i);
    if (!(flags & ECSIMD_HIP_BASE_MGRY)) { xm = fe_from_classical<C>(xm); ym = fe_from_classical<C>(ym); }
  }
  fe nu, de;
  scalar_mult_ladder_x<C>(reinterpret_cast<const uint32_t*>(kodd + (size_t)k_stride * i), xm, ym, nu, de);
  fe_store(num, i, nu); fe_store(den, i, de);
}
// x = num / den in classical form; 0 where the scalar was 0 mod n (and where den = 0: inverse(0) = 0)
__global__ void __launch_bounds__(BLOCK) k_x_finish(const uint64_t* __restrict__ num, const uint64_t* __restrict__ dinv, const uint8_t* __restrict__ state, int state_stride,
                                                    uint64_t* __restrict__ ox, size_t n) {
  const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n) return;
  fe r = fe_to_classical<C>(fe_mul<C>(fe_load(num, i), fe_load(dinv, i)));
  if (state[(size_t)state_stride * i] == 1) {
#pragma unroll
    for (int w = 0; w < 8; ++w) r.w[w] = 0;
  }
  fe_store(ox, i, r);
}
// the lanes k_odd_scalar marked 2 (two scalars out of 2^256: waves without one leave at once): the reference's ladder on
// n - c and a per-lane inversion
__global__ void __launch_bounds__(BLOCK, LADDER_WAVES_PER_SIMD)
k_x_fixup(const uint64_t* __restrict__ kodd, int k_stride, const uint8_t* __restrict__ state, const uint64_t* __restrict__ x, const uint64_t* __restrict__ y,
          uint64_t* __restrict__ ox, size_t n, int flags) {
  const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n || state[k_stride ? i : 0] != 2) return;
  fe xm, ym;
  if (x == nullptr) { xm = fe_from_classical<C>(FE_CONST(C, GX)); ym = fe_from_classical<C>(FE_CONST(C, GY)); }
  else {
    xm = fe_load(x, i); ym = fe_load(y, i);
    if (!(flags & ECSIMD_HIP_BASE_MGRY)) { xm = fe_from_classical<C>(xm); ym = fe_from_classical<C>(ym); }
  }
  const jpoint R = scalar_mult_ladder<C>(reinterpret_cast<const uint32_t*>(kodd + (size_t)k_stride * i), xm, ym);
  fe ax, ay;
  to_affine<C>(R, ax, ay);
  fe_store(ox, i, ax);
}
#endif
}  // namespace

namespace launch {
#ifdef ECS_LADDER_X
// scratch: scalar_mult_x_scratch_bytes(n) bytes, 32-byte aligned.  ox = affine classical x of k*P (k*G for x == nullptr).
template <> void point_launch<C>::scalar_mult_x(hipStream_t s, const uint64_t* k, int k_stride, const uint64_t* x, const uint64_t* y,
                                                uint64_t* ox, uint64_t* scratch, size_t n, int flags) {
  const size_t m = k_stride ? n : 1;                       // scalars: one per element, or one shared
  uint64_t* kodd = scratch; uint64_t* num = kodd + 4 * n; uint64_t* den = num + 4 * n; uint64_t* dinv = den + 4 * n;
  uint8_t* zero = reinterpret_cast<uint8_t*>(dinv + 4 * n);
  hipLaunchKernelGGL(k_odd_scalar, grid_for(m), dim3(BLOCK), 0, s, k, kodd, zero, m);
  hipLaunchKernelGGL(k_scalar_mult_x, grid_for(n), dim3(BLOCK), 0, s, kodd, k_stride, x, y, num, den, n, flags);
  inverse_batched(s, den, dinv, n);
  hipLaunchKernelGGL(k_x_finish, grid_for(n), dim3(BLOCK), 0, s, num, dinv, zero, k_stride ? 1 : 0, ox, n);
  hipLaunchKernelGGL(k_x_fixup, grid_for(n), dim3(BLOCK), 0, s, kodd, k_stride, zero, x, y, ox, n, flags);
}
#endif
template <> void point_launch<C>::scalar_mult(hipStream_t s, const uint64_t* k, int k_stride, const uint64_t* x, const uint64_t* y,
                                              uint64_t* ox, uint64_t* oy, uint64_t* oz, size_t n, int flags) {
  if constexpr (HAS_R29) {
    if (!(flags & ECSIMD_HIP_LADDER_RADIX32)) { hipLaunchKernelGGL(k_scalar_mult<29>, grid_for(n), dim3(BLOCK), 0, s, k, k_stride, x, y, ox, oy, oz, n, flags); return; }
  }
  hipLaunchKernelGGL(k_scalar_mult<32>, grid_for(n), dim3(BLOCK), 0, s, k, k_stride, x, y, ox, oy, oz, n, flags);
}
// ZDAU applied `iters` times in registers (ecsimd_hip_zdau_repeat): the ladder's loop body alone, in either representation.
template <> void point_launch<C>::zdau_repeat(hipStream_t s, const uint64_t* px, const uint64_t* py, const uint64_t* pz, const uint64_t* qx, const uint64_t* qy,
                                              uint64_t* rx, uint64_t* ry, uint64_t* sx, uint64_t* sy, uint64_t* oz, size_t n, int iters, uint64_t swap_bits, int radix) {
  if constexpr (HAS_R29) {
    if (radix == 29) { hipLaunchKernelGGL(k_zdau_repeat<29>, grid_for(n), dim3(BLOCK), 0, s, px, py, pz, qx, qy, rx, ry, sx, sy, oz, n, iters, swap_bits); return; }
  }
  hipLaunchKernelGGL(k_zdau_repeat<32>, grid_for(n), dim3(BLOCK), 0, s, px, py, pz, qx, qy, rx, ry, sx, sy, oz, n, iters, swap_bits);
}
}  // namespace launch
}  // namespace ecsimd_hip
