// k_varwin.inc -- variable-base scalar multiplication with per-lane window tables, for ONE curve
// (included with ECS_CURVE defined).  This is ecsimd_hip_scalar_mult with ECSIMD_HIP_ALG_WINDOWED
// (SURVEY.md 8(b): flags {ALG_REF_LADDER, ALG_WINDOWED}); the reference has only the co-Z ladder
// (curve_group.h:189-218), so parity is affine-level (SURVEY.md 8(a) "level A").
//
// Per lane: a table of 8 affine multiples of P (fast domain, 8 x 64 B contiguous in HBM), then a window loop:
//   P-256 (and secp256k1 with ALG_NO_ENDOMORPHISM): odd digits only -- {1, 3, .., 15}P, 63 x (3 doublings + one fused
//     double-add), ~2 770 field multiplications against the ladder's 4 064 (k_varwin_mult_odd);
//   secp256k1: the GLV split k = k1 + k2*lambda -- {1..8}P, 32 x (4 doublings + 2 checked additions) (k_varwin_mult_glv).
//
// Kernels:
//   k_varwin_odd_multiples / k_varwin_multiples_chain   the table's multiples in Jacobian form -> scratch (SoA, entry-major), each Z the one before
//                        times a stored ratio, the last Z on its own; 1P -> slot 0
//   k_varwin_invert_last + k_varwin_chain_to_table   ONE shared inversion per lane (the chain's last Z), the walk back through the ratios -> table slots 1..7
//   k_varwin_table_iso   secp256k1's default loop: all eight multiples over one Z, no inversion (the loop runs on the isomorphic curve)
//   k_varwin_mult_odd / k_varwin_mult_glv / k_varwin_mult_glv_ct   the window loop, on fe29.cuh's 29-bit limbs; Jacobian result (fast domain) -> scratch,
//                        then the caller runs k_to_affine_batched (k_affine.inc)
// (Rounds 1-3's canonical-word loops and their simultaneous inversion over all 7n Jacobian multiples were measured against these and removed.)
//
// k is reduced mod n first, so the paths are correct for every 256-bit scalar; k = 0 mod n gives Z = 0, which the affine
// conversion turns into (0, 0) like everywhere else in this library.
#include "kernels.h"
#include "point.cuh"
#include "../../include/ecsimd_hip.h"

namespace ecsimd_hip {
namespace {
using launch::BLOCK;
constexpr int C = ECS_CURVE;
constexpr int CI = curve_domain<C>::fast;

ECS_DEV bool vw_is_zero(const fe& a) {
  uint32_t d = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) d |= a.w[i];
  return d == 0;
}

// The window loops run on fe29.cuh's nine signed 29-bit limbs since round 4: jdbl29 / dbl_add29 with lazy limbs, carry passes where a square or
// a wide product needs them and vred29 after every point operation (tools/radix29_model.py prove_window_invariant).  Their tables hold x * 2^261
// (pack29) like the combs'.

ECS_DEV void load_slot(const uint4* __restrict__ table, size_t slot, fe& x, fe& y) {
  const uint4* e = table + slot * 4;
  const uint4 q0 = e[0], q1 = e[1], q2 = e[2], q3 = e[3];
  x.w[0] = q0.x; x.w[1] = q0.y; x.w[2] = q0.z; x.w[3] = q0.w; x.w[4] = q1.x; x.w[5] = q1.y; x.w[6] = q1.z; x.w[7] = q1.w;
  y.w[0] = q2.x; y.w[1] = q2.y; y.w[2] = q2.z; y.w[3] = q2.w; y.w[4] = q3.x; y.w[5] = q3.y; y.w[6] = q3.z; y.w[7] = q3.w;
}
ECS_DEV void store_half_slot(uint4* __restrict__ table, size_t slot, int half, const fe& v) {
  uint4* e = table + slot * 4 + 2 * half;
  e[0] = make_uint4(v.w[0], v.w[1], v.w[2], v.w[3]);
  e[1] = make_uint4(v.w[4], v.w[5], v.w[6], v.w[7]);
}

#ifndef VARWIN_WAVES_PER_SIMD
#define VARWIN_WAVES_PER_SIMD 3   // a cap, not a target: the 29-bit loops need 116 (odd digits) and 106 (GLV) registers and run four waves per SIMD.  (Rounds 1-3,
                                  // canonical words: the GLV loop was capped at 168 with 40 spilled -- 107.7 M/s against 105.5 at 2 waves and no spill,
                                  // profiles/r03/ab_glv_window_kernel.txt.)
#endif
constexpr int VW_ENTRIES = 8;     // {1..8}P (GLV loop) or {1, 3, .., 15}P (odd-digit loop)
constexpr int VW_JAC = 7;         // all but 1P pass through the inversion

// The constant-time GLV loop's table {1..8}P as a CHAIN (round 4): 2P by DBLU, then (m + 1)P = P + mP by co-Z additions, each Z the one before
// times that step's x-difference -- so, as for the odd multiples below, only 8P's Z is inverted (k_varwin_invert_last) and k_varwin_chain_to_table walks
// back through the differences.  6 + 6 x 7 products against rounds 1-3's 4 x 7 + 3 x 11, and the table step costs 5 products per entry against 10.
__global__ void __launch_bounds__(BLOCK) k_varwin_multiples_chain(const uint64_t* __restrict__ x, const uint64_t* __restrict__ y, int flags,
                                                            uint64_t* __restrict__ jx, uint64_t* __restrict__ jy, uint64_t* __restrict__ jh, uint64_t* __restrict__ zlast,
                                                            uint4* __restrict__ table, size_t n) {
  const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n) return;
  fe px = fe_load(x, i), py = fe_load(y, i);
  const bool in_mgry = (flags & ECSIMD_HIP_BASE_MGRY) != 0;
  if constexpr (CI == C) { if (!in_mgry) { px = fe_from_classical<C>(px); py = fe_from_classical<C>(py); } }
  else { if (in_mgry) { px = fe_to_classical<C>(px); py = fe_to_classical<C>(py); } }
  store_half_slot(table, i * VW_ENTRIES, 0, pack29<CI>(px));
  store_half_slot(table, i * VW_ENTRIES, 1, pack29<CI>(py));
  fe ax, ay, z;                                          // (ax, ay) = 2P; (px, py) becomes P over the same z (curve_group.h:64-87 DBLU)
  dblu<CI>(px, py, ax, ay, z);
  fe_store(jx, i, ax); fe_store(jy, i, ay);
#pragma unroll 1
  for (int j = 1; j < VW_JAC; ++j) {                     // (j + 2) P = P + (j + 1) P, co-Z (ZADDU, curve_group.h:91-116: 5M + 2S); P is re-expressed over the new z
    fe rx, ry;
    fe_store(jh, (size_t)j * n + i, fe_sub<CI>(px, ax)); // zaddu's own x1 - x2: the ratio of its Z to the one before
    zaddu<CI>(px, py, ax, ay, z, rx, ry);
    ax = rx; ay = ry;
    fe_store(jx, (size_t)j * n + i, ax); fe_store(jy, (size_t)j * n + i, ay);
  }
  fe_store(zlast, i, z);
}

// ---------------------------------------------------------------- the plain loop with odd digits only
// Regular recoding (Joye-Tunstall): for odd k, digit i = (bits 4i..4i+4 of k, bit 4i forced to 1) - 16 for i < 63 and
// the top digit = (k >> 252) | 1 -- sixty-four ODD digits in [-15, 15], none of them zero, the top one positive.  Exactly
// one of k mod n and n - (k mod n) is odd (n is odd), so every k != 0 mod n has such a form up to the sign of the result.
// No zero digit means no "skip" and no point at infinity inside the loop, and
// the last doubling of every window fuses with the addition (fe29.cuh dbl_add29).  Table: the odd multiples {1, 3, ..., 15}P from one DBLU and seven
// co-Z additions (6 + 7 x 7 = 55 field mults).

// 3P, 5P, ..., 15P (Jacobian) -> jx/jy[j*n + i], j = 0..6; 1P -> table slot 8 i.  A chain (round 4): every Z is the one before times that step's
// x-difference, z_j = z_(j-1) dx_j -- so only the LAST one needs inverting, 1 / z_(j-1) = (1 / z_j) dx_j walks back through the rest: jz[j] takes dx_j,
// zlast[i] the last Z (k_varwin_chain_to_table).
__global__ void __launch_bounds__(BLOCK) k_varwin_odd_multiples(const uint64_t* __restrict__ x, const uint64_t* __restrict__ y, int flags,
                                                                uint64_t* __restrict__ jx, uint64_t* __restrict__ jy, uint64_t* __restrict__ jz, uint64_t* __restrict__ zlast,
                                                                uint4* __restrict__ table, size_t n) {
  const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n) return;
  fe px = fe_load(x, i), py = fe_load(y, i);
  const bool in_mgry = (flags & ECSIMD_HIP_BASE_MGRY) != 0;
  if constexpr (CI == C) { if (!in_mgry) { px = fe_from_classical<C>(px); py = fe_from_classical<C>(py); } }
  else { if (in_mgry) { px = fe_to_classical<C>(px); py = fe_to_classical<C>(py); } }
  store_half_slot(table, i * VW_ENTRIES, 0, pack29<CI>(px));       // the odd-digit loop's table form
  store_half_slot(table, i * VW_ENTRIES, 1, pack29<CI>(py));
  fe dx2, dy2, z;                                          // (dx2, dy2) = 2P; (px, py) becomes P over the same z
  dblu<CI>(px, py, dx2, dy2, z);
  fe ax = px, ay = py;                                     // running odd multiple, co-Z with 2P
#pragma unroll 1
  for (int j = 0; j < VW_JAC; ++j) {                       // (2j + 3) P = (2j + 1) P + 2P; 2P is re-expressed over the new z
    fe rx, ry;
    fe_store(jz, (size_t)j * n + i, fe_sub<CI>(dx2, ax));                // zaddu's own x1 - x2: the ratio of its Z to the one before
    zaddu<CI>(dx2, dy2, ax, ay, z, rx, ry);
    ax = rx; ay = ry;
    fe_store(jx, (size_t)j * n + i, ax); fe_store(jy, (size_t)j * n + i, ay);
  }
  fe_store(zlast, i, z);
}
// The last Z of every lane's chain, inverted together (Montgomery's trick over m lanes' values per GPU lane), in
// the loop's own domain; a zero (an invalid input point) counts as one and comes back as zero.  out: the prefix products on the way up, the inverses on the way down.
__global__ void __launch_bounds__(256) k_varwin_invert_last(const uint64_t* __restrict__ zlast, uint64_t* __restrict__ out, size_t n, size_t lanes, int m) {
  const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= lanes) return;
  const fe one = FE_CONST(CI, R_P);
  fe acc = one;
  for (int j = 0; j < m; ++j) {
    const size_t e = (size_t)j * lanes + g;
    if (e >= n) break;
    fe v = fe_load(zlast, e);
    if (vw_is_zero(v)) v = one;
    acc = fe_mul<CI>(acc, v);
    fe_store(out, e, acc);
  }
  fe inv = fe_inverse<CI>(acc);
  int last = m - 1;
  while (last >= 0 && (size_t)last * lanes + g >= n) --last;
  for (int j = last; j >= 0; --j) {
    const size_t e = (size_t)j * lanes + g;
    fe v = fe_load(zlast, e);
    const bool zero = vw_is_zero(v);
    if (zero) v = one;
    const fe prev = (j > 0) ? fe_load(out, (size_t)(j - 1) * lanes + g) : one;
    fe iv = fe_mul<CI>(inv, prev);
    inv = fe_mul<CI>(inv, v);
    if (zero) {
#pragma unroll
      for (int w = 0; w < 8; ++w) iv.w[w] = 0;
    }
    fe_store(out, e, iv);
  }
}
// One lane, its own seven entries: 1/z of the last from k_varwin_invert_last, back through the x-differences.  The 29-bit loops' table form is
// x * 2^261 mod p canonical (pack29) -- folded into 1/z^2 once per entry (a product by pack29(1)) instead of a product per coordinate.
__global__ void __launch_bounds__(BLOCK) k_varwin_chain_to_table(const uint64_t* __restrict__ jx, const uint64_t* __restrict__ jy, const uint64_t* __restrict__ jdx,
                                                                                         const uint64_t* __restrict__ zinv, uint4* __restrict__ table, size_t n) {
  const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n) return;
  const fe k29 = pack29<CI>(FE_CONST(CI, R_P));
  fe iz = fe_load(zinv, i);
#pragma unroll 1
  for (int j = VW_JAC - 1; j >= 0; --j) {
    const fe X = fe_load(jx, (size_t)j * n + i), Y = fe_load(jy, (size_t)j * n + i);
    const fe iz2 = fe_mul<CI>(fe_sqr<CI>(iz), k29);
    store_half_slot(table, i * VW_ENTRIES + j + 1, 0, fe_mul<CI>(X, iz2));
    store_half_slot(table, i * VW_ENTRIES + j + 1, 1, fe_mul<CI>(Y, fe_mul<CI>(iz2, iz)));
    if (j > 0) iz = fe_mul<CI>(iz, fe_load(jdx, (size_t)j * n + i));
  }
}

// CT (ALG_CONSTANT_TIME on a variable base): the lane's table is the same 8 entries for every window, and every window reads ALL of them --
// 512 contiguous bytes at an address made of the lane index alone -- keeping the wanted one under lane masks.  Four rounds of eight 16-byte
// loads -- two whole entries, ONE 128-byte line (a quarter of every entry per round fetched every line four times: 75 KB per scalar
// multiplication against 32) -- each in flight behind one of the window's four chunks of arithmetic (three doublings, one double-add); the
// first round of the NEXT window is requested before the double-add.  No address, no branch depends on the scalar.
#ifndef VARWIN_CT_WAVES
#define VARWIN_CT_WAVES 3            // 176 registers wanted, 168 to be had at 3 waves: 9 spilled (constant-addressed scratch) and still 70.3 against 68.5 M/s at 2 waves
                                     // (secp256k1 75.8 against 72.9): profiles/r03/ab_constant_time_variable_base.txt
#endif
template <bool CT>
__global__ void __launch_bounds__(BLOCK, CT ? VARWIN_CT_WAVES : VARWIN_WAVES_PER_SIMD) k_varwin_mult_odd(const uint64_t* __restrict__ k, int k_stride, const uint4* __restrict__ table,
                                                              uint64_t* __restrict__ ox, uint64_t* __restrict__ oy, uint64_t* __restrict__ oz, size_t n) {
  const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n) return;
  using O = curve_order<C>;
  fe kk = fe_load(k, k_stride ? i : 0);
  fe order;
#pragma unroll
  for (int j = 0; j < 8; ++j) order.w[j] = O::N[j];
  {                                                     // k mod n (k < 2^256 < 2n)
    fe d;
    const uint32_t borrow = sub8_3(d, kk, order);
    kk = fe_select(borrow, kk, d);
  }
  const bool zero = vw_is_zero(kk);
  const uint32_t flip = 0u - (uint32_t)((kk.w[0] & 1u) == 0u);     // even: use n - k (odd) and negate the result
  {
    fe nk;
    (void)sub8_3(nk, order, kk);
    kk = fe_select(flip, nk, kk);
  }
  if (zero) kk.w[0] = 1;                                // any odd value; the result is replaced by infinity below (a select)
  const size_t base = i * VW_ENTRIES;
  // the accumulator, lazy 29-bit limbs (jdbl29 / dbl_add29); `first` takes the top digit's entry
  struct acc29 { jpoint29 R;
    ECS_DEV void first(const fe& tx, const fe& ty) { R.x = to29(tx); R.y = to29(ty); R.z = fe29_const<r29_consts<CI>::ONE>(); }
    ECS_DEV void dbl() { R = jdbl29<CI>(R); }
    ECS_DEV void dadd(const fe& tx, const fe& ty, uint32_t neg) { R = dbl_add29<CI>(R, to29(tx), cneg29(neg, to29(ty))); }
    ECS_DEV jpoint finish() const { jpoint Q; Q.x = leave29<CI>(R.x); Q.y = leave29<CI>(R.y); Q.z = leave29<CI>(R.z); return Q; } };
  acc29 A;
  uint32_t above = kk.w[7] >> 28;                       // the nibble above the current one (its low bit is the digit's sign)
  if constexpr (CT) {
    const uint4* mine = table + base * 4;               // this lane's 8 entries: 32 x 16 bytes = four 128-byte lines
    uint4 q[8];
    auto request = [&](int pair) {                      // entries 2 pair, 2 pair + 1: ONE line, read once per window
#pragma unroll
      for (int j = 0; j < 8; ++j) q[j] = mine[pair * 8 + j];
      __builtin_amdgcn_sched_barrier(0);               // the loads stay in front of the arithmetic they hide behind
    };
    auto keep = [&](int pair, uint32_t slot, fe& tx, fe& ty) {          // first pair: entry 0 is the default, the others replace it under their masks
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const bool m = (pair == 0 && h == 0) || slot == (uint32_t)(2 * pair + h);
        const uint4 a = q[4 * h], b = q[4 * h + 1], c = q[4 * h + 2], d = q[4 * h + 3];
        tx.w[0] = m ? a.x : tx.w[0]; tx.w[1] = m ? a.y : tx.w[1]; tx.w[2] = m ? a.z : tx.w[2]; tx.w[3] = m ? a.w : tx.w[3];
        tx.w[4] = m ? b.x : tx.w[4]; tx.w[5] = m ? b.y : tx.w[5]; tx.w[6] = m ? b.z : tx.w[6]; tx.w[7] = m ? b.w : tx.w[7];
        ty.w[0] = m ? c.x : ty.w[0]; ty.w[1] = m ? c.y : ty.w[1]; ty.w[2] = m ? c.z : ty.w[2]; ty.w[3] = m ? c.w : ty.w[3];
        ty.w[4] = m ? d.x : ty.w[4]; ty.w[5] = m ? d.y : ty.w[5]; ty.w[6] = m ? d.z : ty.w[6]; ty.w[7] = m ? d.w : ty.w[7];
      }
    };
    {                                                   // top digit = (k >> 252) | 1, positive
      const uint32_t slot = above >> 1;
      fe tx, ty;
      request(0); keep(0, slot, tx, ty); request(1); keep(1, slot, tx, ty);
      request(2); keep(2, slot, tx, ty); request(3); keep(3, slot, tx, ty);
      A.first(tx, ty);
    }
    request(0);
#pragma unroll 1
    for (int w = 62; w >= 0; --w) {
      asm volatile("" : "+s"(w));                       // the window counter stays a scalar register: the exit test is an s_cmp (tools/ct_check.py refuses vcc branches)
#pragma unroll
      for (int j = 7; j > 0; --j) kk.w[j] = __builtin_amdgcn_alignbit(kk.w[j], kk.w[j - 1], 28);   // kk <<= 4
      kk.w[0] <<= 4;
      const uint32_t nib = kk.w[7] >> 28;
      const uint32_t u = nib | 1u;
      const uint32_t neg = 0u - (uint32_t)((above & 1u) == 0u);
      const uint32_t slot = (neg ? 16u - u : u) >> 1;
      above = nib;
      fe tx, ty;
      keep(0, slot, tx, ty); request(1);
      A.dbl();
      keep(1, slot, tx, ty); request(2);
      A.dbl();
      keep(2, slot, tx, ty); request(3);
      A.dbl();
      keep(3, slot, tx, ty); request(0);                // the next window's first line (after the last window: read and dropped)
      A.dadd(tx, ty, neg);
    }
  } else {
  {                                                     // top digit = (k >> 252) | 1, positive
    fe tx, ty;
    load_slot(table, base + (above >> 1), tx, ty);      // ((above | 1) - 1) / 2
    A.first(tx, ty);
  }
  for (int w = 62; w >= 0; --w) {
#pragma unroll
    for (int j = 7; j > 0; --j) kk.w[j] = __builtin_amdgcn_alignbit(kk.w[j], kk.w[j - 1], 28);   // kk <<= 4
    kk.w[0] <<= 4;
    const uint32_t nib = kk.w[7] >> 28;
    const uint32_t u = nib | 1u;                                        // 1, 3, ..., 15
    const uint32_t neg = 0u - (uint32_t)((above & 1u) == 0u);          // digit = u - 16 when the nibble above is even
    const uint32_t mag = neg ? 16u - u : u;
    above = nib;
    fe tx, ty;
    load_slot(table, base + (mag >> 1), tx, ty);                        // in flight during the doublings
    A.dbl(); A.dbl(); A.dbl();
    A.dadd(tx, ty, neg);
  }
  }
  jpoint R = A.finish();
  R.y = fe_select(flip, fe_neg<CI>(R.y), R.y);
  if constexpr (CT) {                                   // k = 0 mod n: infinity, by masks
    const uint32_t keep0 = 0u - (uint32_t)!zero;
#pragma unroll
    for (int j = 0; j < 8; ++j) { R.x.w[j] &= keep0; R.y.w[j] &= keep0; R.z.w[j] &= keep0; }
  } else if (zero) {
#pragma unroll
    for (int j = 0; j < 8; ++j) { R.x.w[j] = 0; R.y.w[j] = 0; R.z.w[j] = 0; }
  }
  fe_store(ox, i, R.x); fe_store(oy, i, R.y); fe_store(oz, i, R.z);
}

// ---------------------------------------------------------------- secp256k1: the GLV endomorphism
// secp256k1 has the endomorphism lambda*(x, y) = (beta*x, y) (beta^3 = 1 mod p, lambda^3 = 1 mod n).  Writing
// k = k1 + k2*lambda (mod n) with |k1|, |k2| < 2^128 halves the doublings: 32 windows x (4 doublings + 2 mixed
// additions + 1 multiplication by beta) ~= 1 800 field multiplications instead of 2 590.  The split is the
// lattice rounding every secp256k1 library uses (constants as published with libsecp256k1; the products are
// small, so exact 256-bit two's-complement arithmetic replaces its mod-n reductions):
//   c1 = round(k*g1 / 2^384), c2 = round(k*g2 / 2^384), k1 = k - c1*a1 - c2*a2, k2 = c1*(-b1) - c2*b2.
// The split returns the representative inside the lattice's fundamental cell, which keeps every prefix away from
// the non-zero lattice vectors, so R = +-T should not occur; the additions are checked all the same (H = 0 switches
// the lane to the tangent or to infinity behind a wave-uniform branch that costs two instructions when not taken).
template <int N> ECS_DEV fe words_fe(const uint32_t (&w)[N]) {
  fe r;
#pragma unroll
  for (int i = 0; i < 8; ++i) r.w[i] = i < N ? w[i] : 0u;
  return r;
}
ECS_DEV fe low_product(const fe& a, const fe& b) {       // a*b mod 2^256
  const fe2 t = mul8x8(a, b);
  fe r;
#pragma unroll
  for (int i = 0; i < 8; ++i) r.w[i] = t.w[i];
  return r;
}
ECS_DEV fe round_shift_384(const fe& k, const fe& g) {   // round(k*g / 2^384), < 2^128
  const fe2 t = mul8x8(k, g);
  uint32_t c0 = t.w[12], c1 = t.w[13], c2 = t.w[14], c3 = t.w[15];
  const uint32_t rnd = t.w[11] >> 31;
  asm("v_add_co_u32 %0, vcc, %0, %4\n\t"
      "v_addc_co_u32 %1, vcc, 0, %1, vcc\n\t"
      "v_addc_co_u32 %2, vcc, 0, %2, vcc\n\t"
      "v_addc_co_u32 %3, vcc, 0, %3, vcc"
      : "+v"(c0), "+v"(c1), "+v"(c2), "+v"(c3) : "v"(rnd) : "vcc");
  fe r;
  r.w[0] = c0; r.w[1] = c1; r.w[2] = c2; r.w[3] = c3; r.w[4] = 0; r.w[5] = 0; r.w[6] = 0; r.w[7] = 0;
  return r;
}
struct glv_consts {
  static constexpr uint32_t G1[8] = {0x45dbb031u, 0xe893209au, 0x71e8ca7fu, 0x3daa8a14u, 0x9284eb15u, 0xe86c90e4u, 0xa7d46bcdu, 0x3086d221u};
  static constexpr uint32_t G2[8] = {0x8ac47f71u, 0x1571b4aeu, 0x9df506c6u, 0x221208acu, 0x0abfe4c4u, 0x6f547fa9u, 0x010e8828u, 0xe4437ed6u};
  static constexpr uint32_t A1[4] = {0x9284eb15u, 0xe86c90e4u, 0xa7d46bcdu, 0x3086d221u};                  // = b2
  static constexpr uint32_t MB1[4] = {0x0abfe4c3u, 0x6f547fa9u, 0x010e8828u, 0xe4437ed6u};                // -b1
  static constexpr uint32_t A2[5] = {0x9d44cfd8u, 0x57c1108du, 0xa8e2f3f6u, 0x14ca50f7u, 0x00000001u};
  static constexpr uint32_t BETA[8] = {0x719501eeu, 0xc1396c28u, 0x12f58995u, 0x9cf04975u, 0xac3434e9u, 0x6e64479eu, 0x657c0710u, 0x7ae96a2bu};
  // beta * 2^261 mod p as nine tight 29-bit limbs (tools/radix29_model.py to_limbs): a compile-time operand of mul29 lives in scalar registers or is
  // rematerialised, where enter29(BETA) held nine vector registers through the loop (tests/test_radix29_model.py checks the value)
  static constexpr int32_t BETA29[9] = {0x103162ff, 0x04361d06, 0x1c057ac5, 0x1858c712, 0x120a07fb, 0x178d02e3, 0x09fc74c4, 0x1af2ecf5, 0x004946d5};
};
// |v| and its sign for a 256-bit two's-complement value
ECS_DEV uint32_t abs256(fe& v) {
  const uint32_t neg = 0u - (v.w[7] >> 31);
  fe z, m;
#pragma unroll
  for (int i = 0; i < 8; ++i) z.w[i] = 0;
  (void)sub8_3(m, z, v);
  v = fe_select(neg, m, v);
  return neg;
}
template <uint32_t HALF = 8u> ECS_DEV void digit_of(uint32_t nib, bool top, uint32_t scalar_neg, uint32_t& mag, uint32_t& neg, uint32_t& skip) {
  if (top) { mag = nib; neg = scalar_neg; }                             // unsigned top digit (0 or 1; up to 8 with 5-bit windows)
  else { mag = nib < HALF ? HALF - nib : nib - HALF; neg = (0u - (uint32_t)(nib < HALF)) ^ scalar_neg; }
  skip = 0u - (uint32_t)(mag == 0u);
}
// ---------------------------------------------------------------- the GLV loop's table without an inversion (round 4)
// All eight multiples over ONE Z, and the loop on the isomorphic curve.  2P = jdbl29(P), (k + 1)P = P + kP by co-Z additions (zaddu29): Z_(k+1) = Z_k dx_k,
// so every multiple's Z divides the last one's, Zg = Z_8, and kP = (X_k f_k^2, Y_k f_k^3) over Zg with f_k = dx_k dx_(k+1) .. dx_7 -- one backward
// walk, 5 products per entry, no inversion, nothing but the lane's own scratch between the lane and its 512 bytes of table.  (x, y) -> (x Zg^2, y Zg^3) maps y^2 = x^3 + b onto
// y^2 = x^3 + b Zg^6: the table's (X_k f_k^2, Y_k f_k^3) are AFFINE points there, the a = 0 doubling and the mixed addition never use b, negation
// and (x, y) -> (beta x, y) commute with the map, and a result (X', Y', Z') of the loop is (X', Y', Z' Zg) on the curve itself: one product at
// the end.  53 + 35 products per lane in one kernel against 61 + 63 in two with 2.4 KB of device-memory traffic per lane between them
// (rounds 1-3's two kernels with a simultaneous inversion: 3.8 of 34 ms at 2^22 lanes).  a != 0 would cost a product per doubling (a Zg^4): secp256k1's
// default loop only.  8 multiples for 4-bit windows: 16 multiples and 5-bit windows -- 26 x (5 doublings + 2 additions) + a 184-product table against
// 33 x (4 + 2) + 88 is 5 % fewer products, and measured 2 % SLOWER, 127.2 against 129.8 M/s: the 1 KB table and its 1.5 KB of scratch cost the table kernel
// more than the loop gains (profiles/r04/README.md); removed.
constexpr int ISO_ENTRIES = 8;                          // {1 .. 8} P: digits are nibble - 8, the top one unsigned and small
template <int ENTRIES> __global__ void __launch_bounds__(BLOCK, 2)
k_varwin_table_iso(const uint64_t* __restrict__ x, const uint64_t* __restrict__ y, int flags, uint4* __restrict__ table, uint64_t* __restrict__ zg, size_t n) {
  constexpr int JAC = ENTRIES - 1;
  const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n) return;
  fe px = fe_load(x, i), py = fe_load(y, i);
  const bool in_mgry = (flags & ECSIMD_HIP_BASE_MGRY) != 0;
  if constexpr (CI == C) { if (!in_mgry) { px = fe_from_classical<C>(px); py = fe_from_classical<C>(py); } }
  else { if (in_mgry) { px = fe_to_classical<C>(px); py = fe_to_classical<C>(py); } }
  const fe29 x1 = enter29<CI>(px), y1 = enter29<CI>(py);
  const size_t base = i * ENTRIES;
  // h[0] = Z_2 (= Z_2 / Z_1), h[k - 1] = Z_(k+1) / Z_k for k = 2..ENTRIES-1; (ex, ey)[k - 2] = kP as born, lazy limbs and all.  Rolled loops, dynamic
  // indices: the three arrays live in scratch (dword-interleaved across the wave: coalesced, unlike the 512-byte-strided table)
  fe29 h[JAC], ex[JAC - 1], ey[JAC - 1];
  jpoint29 Q; Q.x = x1; Q.y = y1; Q.z = fe29_const<r29_consts<CI>::ONE>();
  Q = jdbl29<CI>(Q);                                     // 2P over Z_2
  h[0] = Q.z;
  fe29 qx, qy;                                           // P over the multiple's Z, kept so by zaddu29
  { const fe29 zz = sqr29<CI>(Q.z); qx = mul29<CI>(x1, zz); qy = mul29<CI>(y1, mul29<CI>(zz, Q.z)); }
  fe29 mx = Q.x, my = Q.y, z = Q.z;
#pragma unroll 1
  for (int k = 2; k <= JAC; ++k) {                    // (k + 1)P = P + kP, co-Z (k P = +-P has no solution for these k in a group of prime order)
    ex[k - 2] = mx; ey[k - 2] = my;
    fe29 rx, ry, dx;
    zaddu29<CI>(qx, qy, mx, my, z, rx, ry, dx);
    mx = rx; my = ry;
    h[k - 1] = dx;
  }
  // the last multiple, over Zg = its own Z: a co-Z sum's X = D - W1 - W2 reaches below -p, outside canon29's (-p, 2p): the value reduction first
  store_half_slot(table, base + ENTRIES - 1, 0, canon29<CI>(vred29<CI>(mx))); store_half_slot(table, base + ENTRIES - 1, 1, canon29<CI>(vred29<CI>(my)));
  fe_store(zg, i, canon29<CI>(z));
  fe29 f = h[JAC - 1];
#pragma unroll 1
  for (int k = JAC; k >= 1; --k) {                    // f = f_k
    const fe29 X = (k == 1) ? x1 : ex[k == 1 ? 0 : k - 2], Y = (k == 1) ? y1 : ey[k == 1 ? 0 : k - 2];
    const fe29 f2 = sqr29<CI>(f);
    store_half_slot(table, base + k - 1, 0, canon29<CI>(mul29<CI>(X, f2)));
    store_half_slot(table, base + k - 1, 1, canon29<CI>(mul29<CI>(Y, mul29<CI>(f2, f))));
    if (k > 1) f = mul29<CI>(f, h[k - 2]);
  }
}

// R (+inf flag) += T on fe29.cuh's lazy limbs (round 4), every case handled: R = inf, T skipped, R = T (tangent), R = -T (infinity).  madd29_hr hands out
// H and r, is_zero29 decides "= 0 mod p" on them (a value reduction, one sequential carry pass, an OR: ~45 instructions against the 8-word compare's 9 --
// two per window, beside ~6 500).  Public scalars: the cases are plain divergent control flow -- a skipped digit or a fresh accumulator costs the lane nothing and, unlike a select
// at the end, does not keep the old accumulator alive beside the sum (a third of the loop's registers).
ECS_DEV void add_checked29(jpoint29& R, uint32_t& inf, const fe29& x2, const fe29& y2, uint32_t skip) {
  if (skip) return;
  if (inf) { R.x = x2; R.y = y2; R.z = fe29_const<r29_consts<CI>::ONE>(); inf = 0u; return; }
  fe29 H, r;
  madd29_hr<CI>(R, x2, y2, H, r);
  if (is_zero29<CI>(H)) {                                               // practically never taken
    if (is_zero29<CI>(r)) { jpoint29 T1; T1.x = x2; T1.y = y2; T1.z = fe29_const<r29_consts<CI>::ONE>(); R = jdbl29<CI>(T1); }   // R = T: the tangent
    else inf = ~0u;                                                     // R = -T
    return;
  }
  R = madd29v_finish<CI>(R, H, r);
}
#ifndef VARWIN_GLV_WAVES
#define VARWIN_GLV_WAVES VARWIN_WAVES_PER_SIMD    // (the 29-bit loop needs 106 registers: four waves fit whatever this says)
#endif
// WB: bits per window, 4 (8-entry tables)
template <int WB> __global__ void __launch_bounds__(BLOCK, VARWIN_GLV_WAVES)
k_varwin_mult_glv(const uint64_t* __restrict__ k, int k_stride, const uint4* __restrict__ table, const uint64_t* __restrict__ zg,
                  uint64_t* __restrict__ ox, uint64_t* __restrict__ oy, uint64_t* __restrict__ oz, size_t n) {
  const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n) return;
  using O = curve_order<C>;
  fe kk = fe_load(k, k_stride ? i : 0);
  {
    fe order, d;
#pragma unroll
    for (int j = 0; j < 8; ++j) order.w[j] = O::N[j];
    const uint32_t borrow = sub8_3(d, kk, order);
    kk = fe_select(borrow, kk, d);                      // k mod n
  }
  fe k1, k2;
  {
    const fe c1 = round_shift_384(kk, words_fe(glv_consts::G1));
    const fe c2 = round_shift_384(kk, words_fe(glv_consts::G2));
    fe t;
    (void)sub8_3(t, kk, low_product(c1, words_fe(glv_consts::A1)));
    (void)sub8_3(k1, t, low_product(c2, words_fe(glv_consts::A2)));
    (void)sub8_3(k2, low_product(c1, words_fe(glv_consts::MB1)), low_product(c2, words_fe(glv_consts::A1)));
  }
  const uint32_t s1 = abs256(k1), s2 = abs256(k2);      // |k1|, |k2| < 2^128
  // offset recoding: 32 digits of 4 bits, each (its nibble) - 8 in [-8, 8), under an unsigned top digit (bits 128..131, 0 or 1)
  static_assert(WB == 4, "4-bit windows");
  constexpr int HALF = 1 << (WB - 1), ENTRIES = HALF, WINDOWS = 33;
  constexpr uint32_t DMASK = (1u << WB) - 1u;
  uint32_t u1[5], u2[5];
  {
    fe off;
#pragma unroll
    for (int j = 0; j < 8; ++j) off.w[j] = j < 4 ? 0x88888888u : 0u;
    (void)add8(k1, off); (void)add8(k2, off);
#pragma unroll
    for (int j = 0; j < 5; ++j) { u1[j] = k1.w[j]; u2[j] = k2.w[j]; }
  }
  const size_t base = i * ENTRIES;
  // the accumulator (+ its infinity flag), lazy 29-bit limbs
  struct acc29 { jpoint29 R; uint32_t inf;
    ECS_DEV void init(const fe&) { inf = ~0u;
#pragma unroll
      for (int j = 0; j < R29_LIMBS; ++j) { R.x.l[j] = 0; R.y.l[j] = 0; R.z.l[j] = 0; } }
    ECS_DEV void dbls() {
#pragma unroll
      for (int t = 0; t < WB; ++t) R = jdbl29<CI>(R); }
    ECS_DEV void add(const fe& tx, const fe& ty, uint32_t neg, uint32_t skip, bool lambda) {
      add_checked29(R, inf, lambda ? mul29<CI>(to29(tx), fe29_const<glv_consts::BETA29>()) : to29(tx), cneg29(neg, to29(ty)), skip); }
    // zg: the table's common Z (k_varwin_table_iso) -- the loop ran on the isomorphic curve, (X', Y', Z') there is (X', Y', Z' Zg) here
    ECS_DEV jpoint finish(const uint64_t* zg, size_t i) const { jpoint Q; Q.x = leave29<CI>(R.x); Q.y = leave29<CI>(R.y);
      Q.z = leave29<CI>(zg ? mul29<CI>(R.z, to29(fe_load(zg, i))) : R.z); return Q; } };
  acc29 A;
  A.init(words_fe(glv_consts::BETA));
  for (int w = WINDOWS - 1; w >= 0; --w) {
    const bool top = (w == WINDOWS - 1);
    if (!top) {
#pragma unroll
      for (int j = 4; j > 0; --j) { u1[j] = __builtin_amdgcn_alignbit(u1[j], u1[j - 1], 32 - WB); u2[j] = __builtin_amdgcn_alignbit(u2[j], u2[j - 1], 32 - WB); }
      u1[0] <<= WB; u2[0] <<= WB;
    }
    uint32_t m1, n1, z1, m2, n2, z2;
    digit_of<HALF>(u1[4] & DMASK, top, s1, m1, n1, z1);
    digit_of<HALF>(u2[4] & DMASK, top, s2, m2, n2, z2);
    fe ax, ay, bx, by;
    load_slot(table, base + (m1 == 0u ? 0u : m1 - 1u), ax, ay);         // in flight during the doublings
    if (!top) A.dbls();
    // the second entry is requested AFTER the first addition: no difference either way on 29-bit limbs (123.5 against 123.6 M/s,
    // profiles/r04/ab_glv_default_radix29.txt; on rounds 1-3's canonical words the early request cost 21 more spilled registers); the other waves cover the latency
    A.add(ax, ay, n1, z1, false);
    load_slot(table, base + (m2 == 0u ? 0u : m2 - 1u), bx, by);
    A.add(bx, by, n2, z2, true);                                        // lambda * (x, y) = (beta x, y)
  }
  jpoint R = A.finish(zg, i);
  if (A.inf) {
#pragma unroll
    for (int j = 0; j < 8; ++j) { R.x.w[j] = 0; R.y.w[j] = 0; R.z.w[j] = 0; }
  }
  fe_store(ox, i, R.x); fe_store(oy, i, R.y); fe_store(oz, i, R.z);
}

// Complete mixed addition R = A + B through add_checked29 (the API's Montgomery form in and out): A Jacobian with
// Z = 0 meaning infinity, B affine with (0, 0) meaning infinity.  This is the only caller that drives the tangent
// and the infinity branches of add_checked on purpose.
__global__ void __launch_bounds__(BLOCK) k_add_mixed_complete(const uint64_t* __restrict__ ax, const uint64_t* __restrict__ ay, const uint64_t* __restrict__ az,
                                                              const uint64_t* __restrict__ bx, const uint64_t* __restrict__ by,
                                                              uint64_t* __restrict__ rx, uint64_t* __restrict__ ry, uint64_t* __restrict__ rz, size_t n) {
  const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n) return;
  jpoint R;
  R.x = to_fast<C>(fe_load(ax, i)); R.y = to_fast<C>(fe_load(ay, i)); R.z = to_fast<C>(fe_load(az, i));
  const fe tx = to_fast<C>(fe_load(bx, i)), ty = to_fast<C>(fe_load(by, i));
  uint32_t inf = 0u - (uint32_t)vw_is_zero(R.z);
  const uint32_t skip = 0u - (uint32_t)(vw_is_zero(tx) && vw_is_zero(ty));
  {                                                     // on the 29-bit limbs (both curves: prove_glv_invariant holds for either prime)
    jpoint29 Q; Q.x = enter29<CI>(R.x); Q.y = enter29<CI>(R.y); Q.z = enter29<CI>(R.z);
    add_checked29(Q, inf, enter29<CI>(tx), enter29<CI>(ty), skip);
    R.x = leave29<CI>(Q.x); R.y = leave29<CI>(Q.y); R.z = leave29<CI>(Q.z);
  }
  if (inf) {
#pragma unroll
    for (int j = 0; j < 8; ++j) { R.x.w[j] = 0; R.y.w[j] = 0; R.z.w[j] = 0; }
  }
  fe_store(rx, i, from_fast<C>(R.x)); fe_store(ry, i, from_fast<C>(R.y)); fe_store(rz, i, from_fast<C>(R.z));
}

// ---------------------------------------------------------------- secp256k1: the GLV split in constant time
// ALG_WINDOWED | ALG_CONSTANT_TIME on secp256k1.  The split's digits include zero, and the accumulator is the point at infinity until the first
// non-zero digit (k = 0 mod n: to the end) -- cases the default loop leaves behind a branch (add_checked); a constant-time loop cannot.  A finite
// accumulator never meets R = +-T for a valid point: the split stays inside the lattice's cell (tests/test_recoding_models.py walks every prefix,
// tests/scalar_catalogue.py's aimed scalars included); what does occur is O + T, 2 O, and the sum a zero digit forms with the window's first entry
// and drops, which may be anything.  So this loop runs on the COMPLETE addition law of a
// prime-order curve with a = 0 (Bosma-Lenstra as arranged by Renes, Costello and Batina, "Complete addition formulas for prime order
// elliptic curves", 2016: homogeneous projective (X : Y : Z), x = X/Z, y = Y/Z, O = (0 : 1 : 0)) -- one formula for every pair of
// inputs, a doubling that maps O to O:
//   R + T (T affine):  t0 = X1 x2, t1 = Y1 y2, t3 = (X1 + Y1)(x2 + y2) - t0 - t1, t4 = y2 Z1 + Y1, t5 = x2 Z1 + X1,
//                      A = t1 - 3b Z1, B = t1 + 3b Z1, C = 3b t5:  X3 = t3 A - C t4, Y3 = 3 t0 C + B A, Z3 = t4 B + 3 t0 t3   (11M)
//   2R:                t = 3b Z^2, m = Y^2 - 3t, q = Y^2 + t:  X3 = 2 XY m, Y3 = m q + 8 Y^2 t, Z3 = 8 Y^2 YZ                        (6M + 2S)
// (checked against the affine law on random points, P + P, P + (-P), O + T in the test suite's Python model; 3b = 21 is three shifts and
// two additions).  A zero digit adds the window's first entry and keeps the old sum by a select.  The window's 8 entries {1..8}P are read
// whole, one 128-byte line requested right before each of the four doublings (so that nothing of the table is pending during the two
// additions, where the registers are tightest: 29 spills instead of 53 with a read carried across windows), and BOTH halves' entries are kept from the same read under their own
// masks; lambda (x, y) = (beta x, y).  33 windows x (4 x 8 + 2 x 11 + 1) ~= 1 800 field multiplications, the default GLV loop's count.
// (Round 3 ran these formulas on canonical words, each product reduced on its own: 84.7 M/s at 2^22 lanes, then 86.0 with one reduction per output
// coordinate -- profiles/r04/ab_glv_ct_fused_reductions.txt; ALG_CONSTANT_TIME through the GLV split ran 84.2 against the plain odd-digit loop's 76.0,
// profiles/r03/ab_constant_time_variable_base.txt.  Round 4 moved them to fe29.cuh's 29-bit limbs, pdbl29 / padd29; the other forms were removed.)
#ifndef VARWIN_GLV_CT_WAVES
#define VARWIN_GLV_CT_WAVES 3        // 233 registers wanted; 3 waves (29 spilled -- 32 with the fused reductions --, constant-addressed scratch) beat 2 without spills: 84.6 against 80.4 M/s
#endif
template <int UNUSED> __global__ void __launch_bounds__(BLOCK, VARWIN_GLV_CT_WAVES)
k_varwin_mult_glv_ct(const uint64_t* __restrict__ k, int k_stride, const uint4* __restrict__ table,
                     uint64_t* __restrict__ ox, uint64_t* __restrict__ oy, uint64_t* __restrict__ oz, size_t n) {
  const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n) return;
  using O = curve_order<C>;
  fe kk = fe_load(k, k_stride ? i : 0);
  {
    fe order, d;
#pragma unroll
    for (int j = 0; j < 8; ++j) order.w[j] = O::N[j];
    const uint32_t borrow = sub8_3(d, kk, order);
    kk = fe_select(borrow, kk, d);                      // k mod n
  }
  fe k1, k2;
  {
    const fe c1 = round_shift_384(kk, words_fe(glv_consts::G1));
    const fe c2 = round_shift_384(kk, words_fe(glv_consts::G2));
    fe t;
    (void)sub8_3(t, kk, low_product(c1, words_fe(glv_consts::A1)));
    (void)sub8_3(k1, t, low_product(c2, words_fe(glv_consts::A2)));
    (void)sub8_3(k2, low_product(c1, words_fe(glv_consts::MB1)), low_product(c2, words_fe(glv_consts::A1)));
  }
  const uint32_t s1 = abs256(k1), s2 = abs256(k2);      // |k1|, |k2| < 2^128
  uint32_t u1[5], u2[5];                                // offset recoding over 33 nibbles, as in k_varwin_mult_glv
  {
    fe off;
#pragma unroll
    for (int j = 0; j < 8; ++j) off.w[j] = j < 4 ? 0x88888888u : 0u;
    (void)add8(k1, off); (void)add8(k2, off);
#pragma unroll
    for (int j = 0; j < 5; ++j) { u1[j] = k1.w[j]; u2[j] = k2.w[j]; }
  }
  const uint4* mine = table + i * VW_ENTRIES * 4;       // this lane's 8 entries {1..8}P: four 128-byte lines
  uint4 q[8];
  auto request = [&](int pair) {
#pragma unroll
    for (int j = 0; j < 8; ++j) q[j] = mine[pair * 8 + j];
    __builtin_amdgcn_sched_barrier(0);
  };
  auto keep = [&](int pair, uint32_t slot, fe& tx, fe& ty) {            // entry `slot` (0..7); pair 0 sets the default, entry 0
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const bool m = (pair == 0 && h == 0) || slot == (uint32_t)(2 * pair + h);
      const uint4 a = q[4 * h], b = q[4 * h + 1], c = q[4 * h + 2], d = q[4 * h + 3];
      tx.w[0] = m ? a.x : tx.w[0]; tx.w[1] = m ? a.y : tx.w[1]; tx.w[2] = m ? a.z : tx.w[2]; tx.w[3] = m ? a.w : tx.w[3];
      tx.w[4] = m ? b.x : tx.w[4]; tx.w[5] = m ? b.y : tx.w[5]; tx.w[6] = m ? b.z : tx.w[6]; tx.w[7] = m ? b.w : tx.w[7];
      ty.w[0] = m ? c.x : ty.w[0]; ty.w[1] = m ? c.y : ty.w[1]; ty.w[2] = m ? c.z : ty.w[2]; ty.w[3] = m ? c.w : ty.w[3];
      ty.w[4] = m ? d.x : ty.w[4]; ty.w[5] = m ? d.y : ty.w[5]; ty.w[6] = m ? d.z : ty.w[6]; ty.w[7] = m ? d.w : ty.w[7];
    }
  };
  // the accumulator, lazy 29-bit limbs; O = (0 : 1 : 0)
  struct acc29 { jpoint29 R;
    ECS_DEV void init() {
#pragma unroll
      for (int j = 0; j < R29_LIMBS; ++j) { R.x.l[j] = 0; R.z.l[j] = 0; }
      R.y = fe29_const<r29_consts<CI>::ONE>(); }
    ECS_DEV void dbl() { R = pdbl29<CI>(R); }
    ECS_DEV void add(const fe& tx, const fe& ty, uint32_t neg, uint32_t zero, bool lambda) {
      const fe29 x2 = lambda ? mul29<CI>(to29(tx), fe29_const<glv_consts::BETA29>()) : to29(tx);
      const jpoint29 S = padd29<CI>(R, x2, cneg29(neg, to29(ty)));
      R.x = select29(zero, R.x, S.x); R.y = select29(zero, R.y, S.y); R.z = select29(zero, R.z, S.z); }
    ECS_DEV void store(uint64_t* ox, uint64_t* oy, uint64_t* oz, size_t i) const {
      const fe29 Zn = norm29(R.z), zz = sqr29<CI>(Zn);
      fe_store(ox, i, leave29<CI>(mul29<CI>(R.x, Zn))); fe_store(oy, i, leave29<CI>(mul29<CI>(R.y, zz))); fe_store(oz, i, leave29<CI>(Zn)); } };
  acc29 A;
  A.init();
#pragma unroll 1
  for (int w = 32; w >= 0; --w) {
    asm volatile("" : "+s"(w));                         // the window counter stays a scalar register (tools/ct_check.py)
    const bool top = (w == 32);
    if (!top) {
#pragma unroll
      for (int j = 4; j > 0; --j) { u1[j] = __builtin_amdgcn_alignbit(u1[j], u1[j - 1], 28); u2[j] = __builtin_amdgcn_alignbit(u2[j], u2[j - 1], 28); }
      u1[0] <<= 4; u2[0] <<= 4;
    }
    uint32_t m1, n1, z1, m2, n2, z2;
    digit_of(u1[4] & 15u, top, s1, m1, n1, z1);
    digit_of(u2[4] & 15u, top, s2, m2, n2, z2);
    const uint32_t e1 = z1 ? 0u : m1 - 1u, e2 = z2 ? 0u : m2 - 1u;     // a zero digit reads entry 0 and drops the sum below
    fe ax, ay, bx, by;                                  // four lines, each in flight behind one doubling; nothing of the table is pending during the additions
    request(0);
    A.dbl();                                            // (the top window doubles O four times: O)
    keep(0, e1, ax, ay); keep(0, e2, bx, by); request(1);
    A.dbl();
    keep(1, e1, ax, ay); keep(1, e2, bx, by); request(2);
    A.dbl();
    keep(2, e1, ax, ay); keep(2, e2, bx, by); request(3);
    A.dbl();
    keep(3, e1, ax, ay); keep(3, e2, bx, by);
    A.add(ax, ay, n1, z1, false);
    A.add(bx, by, n2, z2, true);                        // lambda * (x, y) = (beta x, y)
  }
  // (X : Y : Z) -> the Jacobian triple of the same point over the same Z, which k_to_affine_batched expects: (X Z, Y Z^2, Z); O -> Z = 0
  A.store(ox, oy, oz, i);
}
}  // namespace

namespace launch {
template <> void point_launch<C>::varwin_scalar_mult(hipStream_t s, const uint64_t* k, int k_stride, const uint64_t* x, const uint64_t* y, int flags,
                                                     uint64_t* scratch, uint64_t* ox, uint64_t* oy, size_t n) {
  // scratch: 7n x 4 field elements (the chain's multiples, ratios and last Z; reused for the Jacobian result) + 8n x 64 B table
  uint64_t* jx = scratch; uint64_t* jy = jx + 4 * (size_t)VW_JAC * n; uint64_t* jz = jy + 4 * (size_t)VW_JAC * n;
  uint64_t* zlast = jz + 4 * (size_t)VW_JAC * n; uint64_t* zinv = zlast + 4 * n;
  uint4* table = reinterpret_cast<uint4*>(zlast + 4 * (size_t)VW_JAC * n);
  uint64_t* rx = jx; uint64_t* ry = jx + 4 * n; uint64_t* rz = jx + 8 * n;            // the Jacobian result, once the multiples are dead
  const bool ct = (flags & ECSIMD_HIP_ALG_CONSTANT_TIME) != 0;           // every entry of the lane's table read in every window
  // the multiples' Z form a chain: ONE inversion per lane's last Z, the rest by the walk back (k_varwin_chain_to_table)
  auto chain_to_table = [&]() {
    size_t m = n >> 17; if (m < 1) m = 1; if (m > 256) m = 256;
    const size_t ilanes = (n + m - 1) / m;
    hipLaunchKernelGGL(k_varwin_invert_last, dim3((unsigned)((ilanes + 255) / 256)), dim3(256), 0, s, zlast, zinv, n, ilanes, (int)m);
    hipLaunchKernelGGL(k_varwin_chain_to_table, grid_for(n), dim3(BLOCK), 0, s, jx, jy, jz, zinv, table, n);
  };
  if constexpr (C == CURVE_SECP256K1) {
    if (!(flags & ECSIMD_HIP_ALG_NO_ENDOMORPHISM)) {                       // the GLV split
      if (!ct) {
        // the table over one Z, the loop on the isomorphic curve: no inversion, no second table kernel.  Its own layout: the Jacobian result (12n words),
        // Zg (4n), then the table of ISO_ENTRIES x 64 B per lane -- 128 + 512 bytes per lane of the 1 408 there are
        static_assert(16 * 8 + ISO_ENTRIES * 64 <= 7 * 4 * 32 + 8 * 64, "kernels.h varwin_scratch_bytes");
        uint64_t* zg = jx + 12 * n;
        uint4* itable = reinterpret_cast<uint4*>(jx + 16 * n);
        hipLaunchKernelGGL(k_varwin_table_iso<ISO_ENTRIES>, grid_for(n), dim3(BLOCK), 0, s, x, y, flags, itable, zg, n);
        hipLaunchKernelGGL(k_varwin_mult_glv<4>, grid_for(n), dim3(BLOCK), 0, s, k, k_stride, (const uint4*)itable, (const uint64_t*)zg, rx, ry, rz, n);
      } else {
        hipLaunchKernelGGL(k_varwin_multiples_chain, grid_for(n), dim3(BLOCK), 0, s, x, y, flags, jx, jy, jz, zlast, table, n);       // {1..8}P
        chain_to_table();
        hipLaunchKernelGGL(k_varwin_mult_glv_ct<0>, grid_for(n), dim3(BLOCK), 0, s, k, k_stride, table, rx, ry, rz, n);
      }
      to_affine_batched(s, rx, ry, rz, ox, oy, n, true);
      return;
    }
  }
  hipLaunchKernelGGL(k_varwin_odd_multiples, grid_for(n), dim3(BLOCK), 0, s, x, y, flags, jx, jy, jz, zlast, table, n);              // {1,3,..,15}P
  chain_to_table();
  if (ct) hipLaunchKernelGGL(k_varwin_mult_odd<true>, grid_for(n), dim3(BLOCK), 0, s, k, k_stride, table, rx, ry, rz, n);
  else hipLaunchKernelGGL(k_varwin_mult_odd<false>, grid_for(n), dim3(BLOCK), 0, s, k, k_stride, table, rx, ry, rz, n);
  to_affine_batched(s, rx, ry, rz, ox, oy, n, true);
}
template <> void point_launch<C>::add_mixed_complete(hipStream_t s, const uint64_t* ax, const uint64_t* ay, const uint64_t* az, const uint64_t* bx, const uint64_t* by,
                                                     uint64_t* rx, uint64_t* ry, uint64_t* rz, size_t n) {
  hipLaunchKernelGGL(k_add_mixed_complete, grid_for(n), dim3(BLOCK), 0, s, ax, ay, az, bx, by, rx, ry, rz, n);
}
}  // namespace launch
}  // namespace ecsimd_hip
