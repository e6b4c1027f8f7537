// k_affine.inc -- batched Jacobian -> affine conversion and the fixed-base windowed multiplication,
// for ONE curve (included with ECS_CURVE defined).
//
// 1. k_to_affine_batched: Montgomery's simultaneous inversion.  The reference inverts every lane's Z
//    on its own (jacobian_curve_point.h:33-42 -> gfp.h:42-44: 255 S + 128 M per lane, SURVEY.md 8(f)
//    rank 1).  Here a lane owns M elements (strided so that loads stay coalesced), multiplies their Z
//    together, inverts ONCE, and walks back: 7 field mults per element + 267/M (one addition-chain inversion, point.cuh).  The inverse of a
//    field element is unique, so x = X/Z^2, y = Y/Z^3 are bit-identical to the reference's.
//    Z = 0 (the ladder's degenerate outputs) yields (0, 0), as 0^(p-2) = 0 does in the reference.
//    y == nullptr: the x coordinate only.
// 2. k_base_windowed: k*G with 4-bit windows.  64 tables x 16 entries x 64 B of affine multiples
//    d*16^w*G staged in LDS (64 KiB per workgroup), one mixed addition (curve_group.h:155-179
//    ADD_Z2_1 formula) per window (computed with the 8M + 3S form madd_hmv).  This is BASELINE.json configs[2]; the reference has no such
//    algorithm, so it is parity-checked at the affine level only (SURVEY.md 8(a) "level A").
#include "kernels.h"
#include "point.cuh"

namespace ecsimd_hip {
namespace {
constexpr int C = ECS_CURVE;
constexpr int CI = curve_domain<C>::fast;
constexpr size_t BATCH_INVERSION_MAX = 128;      // elements that share one inversion (one lane's strided slice)

ECS_DEV bool fe_is_zero(const fe& a) {
  uint32_t d = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) d |= a.w[i];
  return d == 0;
}
// all ones where a == 0, as DATA (not a branch condition): the simultaneous inversions below also run on the Jacobian k G of an ECDSA signature, whose Z is
// as secret as the nonce -- their zero handling is selects (tools/ct_check.py check_secret_flow holds the shipped ISA to it)
ECS_DEV uint32_t fe_zero_mask(const fe& a) {
  uint32_t d = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) d |= a.w[i];
  return (uint32_t)((int32_t)((d | (0u - d)) ^ 0x80000000u) >> 31);       // d == 0  <=>  bit 31 of d | -d is clear
}
ECS_DEV fe fe_and_not(const fe& a, uint32_t m) { fe r;
#pragma unroll
  for (int i = 0; i < 8; ++i) r.w[i] = a.w[i] & ~m;
  return r; }

// ---------------------------------------------------------------- the combs' accumulator (round 4)
// Every fixed-base comb (k_base_windowed, k_base_windowed_s, k_base_windowed_g) is "start from one table entry, add the others, hand the Jacobian
// sum to k_to_affine_batched".  comb_acc<RADIX> is the representation the additions run in: 29 = fe29.cuh's nine signed 29-bit limbs (madd29:
// carry-free columns, lazy limbs, three carry passes per addition; bounds proven by tools/radix29_model.py prove_comb_invariant), 32 = field.cuh's
// canonical words (madd_hmv, rounds 1-3).  The table keeps 64-byte entries either way: with radix 29 a coordinate is stored as the canonical residue
// of x * 2^261 (pack29 at build time) and unpacked to tight limbs by shifts and masks at the read (to29).  The sums are the same points; the Jacobian
// representative is free at the affine level (SURVEY.md 8(a) level A).  The LDS combs sum on 29-bit limbs (round 4; canonical words removed).
template <int RADIX> struct comb_acc;
template <> struct comb_acc<32> {
  jpoint A;
  static ECS_DEV fe pack(const fe& fast) { return fast; }
  ECS_DEV void start(const fe& tx, const fe& ty, uint32_t neg) { A.x = tx; A.y = fe_select(neg, fe_neg<CI>(ty), ty); A.z = FE_CONST(CI, R_P); }
  ECS_DEV void add(const fe& tx, const fe& ty, uint32_t neg) { A = madd_hmv<CI>(A.x, A.y, A.z, tx, fe_select(neg, fe_neg<CI>(ty), ty)); }
  ECS_DEV void take(uint32_t m, const fe& tx, const fe& ty) { A.x = fe_select(m, tx, A.x); A.y = fe_select(m, ty, A.y); A.z = fe_select(m, FE_CONST(CI, R_P), A.z); }
  ECS_DEV jpoint finish() const { return A; }
};
template <> struct comb_acc<29> {
  jpoint29 A;
  static ECS_DEV fe pack(const fe& fast) { return pack29<CI>(fast); }
  ECS_DEV void start(const fe& tx, const fe& ty, uint32_t neg) { A.x = to29(tx); A.y = cneg29(neg, to29(ty)); A.z = fe29_const<r29_consts<CI>::ONE>(); }
  ECS_DEV void add(const fe& tx, const fe& ty, uint32_t neg) { A = madd29<CI>(A, to29(tx), cneg29(neg, to29(ty))); }
  ECS_DEV void take(uint32_t m, const fe& tx, const fe& ty) {
    A.x = select29(m, to29(tx), A.x); A.y = select29(m, to29(ty), A.y); A.z = select29(m, fe29_const<r29_consts<CI>::ONE>(), A.z); }
  ECS_DEV jpoint finish() const { jpoint R; R.x = leave29<CI>(A.x); R.y = leave29<CI>(A.y); R.z = leave29<CI>(A.z); return R; }
};
using comb = comb_acc<29>;
// The 20-bit comb in device memory is 12 additions behind 13 random table reads: the radix-29 form's boundary work (three leave29 products and
// the unpacking) costs what its cheaper additions save at 2^22 lanes and loses 6 % at 2^24 (1 313 against 1 405 M/s, profiles/r04/README.md):
// that kernel and its table keep the canonical words.
using comb_big = comb_acc<32>;

// IN_FAST: the Jacobian input is already in the fast domain (internal callers); otherwise it is in
// the API's Montgomery form.  x[] doubles as scratch for the prefix products, so x/y must not alias
// the inputs (the launcher checks).
template <bool IN_FAST>
__global__ void __launch_bounds__(256) k_to_affine_batched(const uint64_t* __restrict__ jx, const uint64_t* __restrict__ jy, const uint64_t* __restrict__ jz,
                                                            uint64_t* __restrict__ x, uint64_t* __restrict__ y, size_t n, size_t lanes, int m) {
  const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= lanes) return;
  const fe one = FE_CONST(CI, R_P);
  fe acc = one;
  for (int j = 0; j < m; ++j) {                       // prefix products p_j = z_0 ... z_j  -> x[e_j]
    const size_t e = (size_t)j * lanes + g;
    if (e >= n) break;
    fe z = fe_load(jz, e);
    if constexpr (!IN_FAST) z = to_fast<C>(z);
    z = fe_select(fe_zero_mask(z), one, z);
    acc = fe_mul<CI>(acc, z);
    fe_store(x, e, acc);
  }
  fe inv = fe_inverse<CI>(acc);                       // one inversion per lane
  int last = m - 1;
  while (last >= 0 && (size_t)last * lanes + g >= n) --last;
  for (int j = last; j >= 0; --j) {
    const size_t e = (size_t)j * lanes + g;
    fe z = fe_load(jz, e), X = fe_load(jx, e);
    if constexpr (!IN_FAST) { z = to_fast<C>(z); X = to_fast<C>(X); }
    const uint32_t zero = fe_zero_mask(z);
    z = fe_select(zero, one, z);
    const fe prev = (j > 0) ? fe_load(x, (size_t)(j - 1) * lanes + g) : one;
    fe iz = fe_mul<CI>(inv, prev);                    // 1 / z_j
    inv = fe_mul<CI>(inv, z);                         // 1 / (z_0 ... z_(j-1))
    iz = fe_and_not(iz, zero);                        // reference: inverse(0) = 0^(p-2) = 0
    const fe iz2 = fe_sqr<CI>(iz);
    fe_store(x, e, fast_to_classical<C>(fe_mul<CI>(X, iz2)));
    if (y != nullptr) {                               // x-coordinate-only callers (ECDH, ECDSA's r) pass no y: 5 field mults instead of 7, 32 B less each way
      fe Y = fe_load(jy, e);
      if constexpr (!IN_FAST) Y = to_fast<C>(Y);
      fe_store(y, e, fast_to_classical<C>(fe_mul<CI>(Y, fe_mul<CI>(iz2, iz))));
    }
  }
}

// The last step of an ECDSA verification: ok[i] = finite[i] && (x[i] mod n == r[i]), x classical in [0, p), n < p < 2n.
__global__ void __launch_bounds__(256) k_x_mod_n_equals(const uint64_t* __restrict__ x, const uint8_t* __restrict__ finite, const uint64_t* __restrict__ r,
                                                        uint8_t* __restrict__ ok, size_t n) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const fe v = fe_load(x, i);
  fe order, d;
#pragma unroll
  for (int j = 0; j < 8; ++j) order.w[j] = curve_order<C>::N[j];
  const uint32_t borrow = sub8_3(d, v, order);            // x < n: keep x
  const fe red = fe_select(borrow, v, d);
  ok[i] = (uint8_t)(finite[i] != 0 && fe_eq(red, fe_load(r, i)));
}

// GFp::inverse over a batch (gfp.h:42-44) with the same trick: out[] holds the prefix products on the way up and the
// inverses on the way down, so out must not alias a (the launcher falls back to the per-element kernel if it does).
// Montgomery form in and out; 0 maps to 0 like the reference's a^(p-2).
__global__ void __launch_bounds__(256) k_inverse_batched(const uint64_t* __restrict__ a, uint64_t* __restrict__ out, size_t n, size_t lanes, int m) {
  const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= lanes) return;
  const fe one = FE_CONST(CI, R_P);
  fe acc = one;
  for (int j = 0; j < m; ++j) {
    const size_t e = (size_t)j * lanes + g;
    if (e >= n) break;
    fe v = to_fast<C>(fe_load(a, e));
    v = fe_select(fe_zero_mask(v), one, v);
    acc = fe_mul<CI>(acc, v);
    fe_store(out, e, acc);
  }
  fe inv = fe_inverse<CI>(acc);
  int last = m - 1;
  while (last >= 0 && (size_t)last * lanes + g >= n) --last;
  for (int j = last; j >= 0; --j) {
    const size_t e = (size_t)j * lanes + g;
    fe v = to_fast<C>(fe_load(a, e));
    const uint32_t zero = fe_zero_mask(v);
    v = fe_select(zero, one, v);
    const fe prev = (j > 0) ? fe_load(out, (size_t)(j - 1) * lanes + g) : one;
    fe iv = fe_mul<CI>(inv, prev);
    inv = fe_mul<CI>(inv, v);
    fe_store(out, e, from_fast<C>(fe_and_not(iv, zero)));
  }
}

// Batched affine addition R = A + B (classical coordinates in and out) with ONE inversion per lane:
// the denominators of the chord / tangent slopes are inverted together.  (0, 0) encodes the point at
// infinity (it is on neither curve: b != 0); finite[i] = 0 marks an infinite result.  This is the last
// step of u1*G + u2*Q (SURVEY.md 8(f) rank 4): the two products come from the windowed fixed-base
// kernel and the ladder, both already affine through the simultaneous-inversion kernel.
__global__ void __launch_bounds__(256) k_affine_add_batched(const uint64_t* __restrict__ ax, const uint64_t* __restrict__ ay,
                                                            const uint64_t* __restrict__ bx, const uint64_t* __restrict__ by,
                                                            uint64_t* __restrict__ rx, uint64_t* __restrict__ ry, uint8_t* __restrict__ finite,
                                                            size_t n, size_t lanes, int m) {
  const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= lanes) return;
  const fe one = FE_CONST(CI, R_P);
  fe acc = one;
  // pass 1: denominators (x2 - x1, or 2*y1 for a doubling, or 1 where no slope is needed); prefix products -> rx
  for (int j = 0; j < m; ++j) {
    const size_t e = (size_t)j * lanes + g;
    if (e >= n) break;
    const fe x1 = classical_to_fast<C>(fe_load(ax, e)), y1 = classical_to_fast<C>(fe_load(ay, e));
    const fe x2 = classical_to_fast<C>(fe_load(bx, e)), y2 = classical_to_fast<C>(fe_load(by, e));
    const bool inf1 = fe_is_zero(x1) && fe_is_zero(y1), inf2 = fe_is_zero(x2) && fe_is_zero(y2);
    const bool same_x = fe_eq(x1, x2), same_y = fe_eq(y1, y2);
    fe den = fe_sub<CI>(x2, x1);
    if (same_x) den = fe_dbl<CI>(y1);                          // tangent (P == Q); P == -Q is handled in pass 2
    if (inf1 || inf2 || (same_x && !same_y) || fe_is_zero(den)) den = one;
    acc = fe_mul<CI>(acc, den);
    fe_store(rx, e, acc);
  }
  fe inv = fe_inverse<CI>(acc);
  int last = m - 1;
  while (last >= 0 && (size_t)last * lanes + g >= n) --last;
  for (int j = last; j >= 0; --j) {
    const size_t e = (size_t)j * lanes + g;
    const fe x1 = classical_to_fast<C>(fe_load(ax, e)), y1 = classical_to_fast<C>(fe_load(ay, e));
    const fe x2 = classical_to_fast<C>(fe_load(bx, e)), y2 = classical_to_fast<C>(fe_load(by, e));
    const bool inf1 = fe_is_zero(x1) && fe_is_zero(y1), inf2 = fe_is_zero(x2) && fe_is_zero(y2);
    const bool same_x = fe_eq(x1, x2), same_y = fe_eq(y1, y2);
    fe den = fe_sub<CI>(x2, x1), num = fe_sub<CI>(y2, y1);
    if (same_x) {                                              // tangent slope (3 x^2 + a) / (2 y)
      den = fe_dbl<CI>(y1);
      const fe xx = fe_sqr<CI>(x1);
      num = fe_add<CI>(fe_dbl<CI>(xx), xx);
      if constexpr (C == CURVE_P256) num = fe_add<CI>(num, FE_CONST(CI, AM));
    }
    const bool no_slope = inf1 || inf2 || (same_x && !same_y) || fe_is_zero(den);
    if (no_slope) den = one;
    const fe prev = (j > 0) ? fe_load(rx, (size_t)(j - 1) * lanes + g) : one;
    const fe iden = fe_mul<CI>(inv, prev);
    inv = fe_mul<CI>(inv, den);
    const fe lam = fe_mul<CI>(num, iden);
    fe x3 = fe_sub<CI>(fe_sub<CI>(fe_sqr<CI>(lam), x1), x2);
    fe y3 = fe_sub<CI>(fe_mul<CI>(lam, fe_sub<CI>(x1, x3)), y1);
    bool fin = true;
    if (inf1) { x3 = x2; y3 = y2; fin = !inf2; }
    else if (inf2) { x3 = x1; y3 = y1; }
    else if (no_slope) {                                       // P == -Q (or a 2-torsion tangent): infinity
#pragma unroll
      for (int i = 0; i < 8; ++i) { x3.w[i] = 0; y3.w[i] = 0; }
      fin = false;
    }
    fe_store(rx, e, fast_to_classical<C>(x3));
    if (ry) fe_store(ry, e, fast_to_classical<C>(y3));
    if (finite) finite[e] = (uint8_t)fin;
  }
}

// Table entry (w, d), affine, fast domain: 16 words {x[8], y[8]} at T[(w*E + d)*16], E = launch::FIXED4_ENTRIES: (2d + 1) * 16^w * G, d = 0..7.
constexpr int WINDOWS = 64, W4E = launch::FIXED4_ENTRIES, TABLE_WORDS = WINDOWS * W4E * 16;          // 32 768 B
__global__ void __launch_bounds__(256) k_pack_table(const uint64_t* __restrict__ tx, const uint64_t* __restrict__ ty, uint32_t* __restrict__ table) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= WINDOWS * W4E + 1) return;                             // + the point of k* (comb_special)
  fe x = fe_load(tx, e), y = fe_load(ty, e);           // classical affine from the ladder kernel
  x = comb::pack(classical_to_fast<C>(x)); y = comb::pack(classical_to_fast<C>(y));
#pragma unroll
  for (int i = 0; i < 8; ++i) { table[e * 16 + i] = x.w[i]; table[e * 16 + 8 + i] = y.w[i]; }
}

#ifndef ECS_WBLOCK
#define ECS_WBLOCK 256               // with the 32 KiB table of odd multiples four (P-256, 122 VGPRs) or three (secp256k1, 146) workgroups share a CU;
#endif                               // 512 threads left secp256k1 with ONE workgroup per CU (2 waves per SIMD): profiles/r03/ab_fixed_base_workgroup_size_odd_digits.txt
constexpr int WBLOCK = ECS_WBLOCK;   // the waves of a workgroup share one LDS copy of the table
ECS_DEV void lds_entry(const uint4* e, fe& tx, fe& ty) {
  const uint4 q0 = e[0], q1 = e[1], q2 = e[2], q3 = e[3];
  tx.w[0] = q0.x; tx.w[1] = q0.y; tx.w[2] = q0.z; tx.w[3] = q0.w; tx.w[4] = q1.x; tx.w[5] = q1.y; tx.w[6] = q1.z; tx.w[7] = q1.w;
  ty.w[0] = q2.x; ty.w[1] = q2.y; ty.w[2] = q2.z; ty.w[3] = q2.w; ty.w[4] = q3.x; ty.w[5] = q3.y; ty.w[6] = q3.z; ty.w[7] = q3.w;
}
// The one scalar an odd-digit comb cannot add up: at its LAST mixed addition the accumulator can EQUAL the table point (R = T, the chord
// formula degenerates).  With B = 2^bits and S the sum of the other windows' terms, R = T means S = d B^w (mod n) for the last term; S is
// a multiple of a power of B next to k < n, so the only solutions are S = n + d_0 for the high-to-low order -- k* = n - 2 (n mod B), and
// only when k*'s recoding gives d_0 = -(n mod B) -- and d B^w - S = n for the low-to-high order -- k* = n - 2 (n mod B^w), w the top window.
// ONE odd scalar per curve and kernel (and the even n - k*, which the k -> n - k flip maps onto it): P-256 with 4-bit windows k = +-2 --
// that is how round 3's test found it -- and with the 20-bit windows, on both curves, k = +-(n - 2 (n mod 2^240)), which had been there
// since round 1.  Every other addition of the comb is exception-free, and R = -T cannot occur for k != 0 mod n (DESIGN.md section 5).
// The host computes k* and k* G with the ladder when it builds the table (capi.hip ensure_window_table) and appends them to it:
//   table[entries] = k* G (x, y; fast domain),  table[entries + 1] = {k* (8 words), 0...}   (k* = 0: this kernel has no such scalar).
// A lane whose recoded scalar equals k* takes that point instead of its sum, behind a wave-uniform branch (public-scalar algorithms).
ECS_DEV uint32_t comb_special(const fe& kf, const uint4* __restrict__ tail) {              // tail = &table[(entries + 1) * 4]
  const uint4 a = tail[0], b = tail[1];
  const uint32_t d = (kf.w[0] ^ a.x) | (kf.w[1] ^ a.y) | (kf.w[2] ^ a.z) | (kf.w[3] ^ a.w) | (kf.w[4] ^ b.x) | (kf.w[5] ^ b.y) | (kf.w[6] ^ b.z) | (kf.w[7] ^ b.w);
  return 0u - (uint32_t)(d == 0u);
}
// ALG_CONSTANT_TIME: every lane reads ALL entries of the window -- one address for the whole wave, an LDS broadcast -- and keeps its own under
// lane masks: no address and no branch depends on the scalar (tools/ct_check.py checks the shipped ISA).
template <int ENTRIES> ECS_DEV void lds_entry_scan(const uint4* win, uint32_t slot, fe& tx, fe& ty) {
  lds_entry(win, tx, ty);
#pragma unroll
  for (int e = 1; e < ENTRIES; ++e) {
    fe ex, ey;
    lds_entry(win + e * 4, ex, ey);
    const uint32_t m = 0u - (uint32_t)(slot == (uint32_t)e);
    tx = fe_select(m, ex, tx); ty = fe_select(m, ey, ty);
  }
}
template <bool CT = false, class ACC> ECS_DEV void comb_take_special(uint32_t special, const uint4* __restrict__ entry, ACC& A) {   // entry = &table[entries * 4]
  if (CT || __builtin_amdgcn_ballot_w64(special != 0u) != 0ull) {                                   // constant time: taken by every wave
    const uint4 q0 = entry[0], q1 = entry[1], q2 = entry[2], q3 = entry[3];
    fe tx, ty;
    tx.w[0] = q0.x; tx.w[1] = q0.y; tx.w[2] = q0.z; tx.w[3] = q0.w; tx.w[4] = q1.x; tx.w[5] = q1.y; tx.w[6] = q1.z; tx.w[7] = q1.w;
    ty.w[0] = q2.x; ty.w[1] = q2.y; ty.w[2] = q2.z; ty.w[3] = q2.w; ty.w[4] = q3.x; ty.w[5] = q3.y; ty.w[6] = q3.z; ty.w[7] = q3.w;
    A.take(special, tx, ty);
  }
}
template <bool CT> __global__ void __launch_bounds__(WBLOCK) k_base_windowed(const uint64_t* __restrict__ k, const uint32_t* __restrict__ table,
                                                          uint64_t* __restrict__ ox, uint64_t* __restrict__ oy, uint64_t* __restrict__ oz, size_t n) {
  __shared__ uint4 lds[TABLE_WORDS / 4];
  {
    const uint4* src = reinterpret_cast<const uint4*>(table);
    for (int e = threadIdx.x; e < TABLE_WORDS / 4; e += WBLOCK) lds[e] = src[e];
  }
  __syncthreads();
  const size_t i = (size_t)blockIdx.x * WBLOCK + threadIdx.x;
  if (i >= n) return;
  // Regular recoding with odd digits (Joye-Tunstall), the scheme of k_base_windowed_g and k_varwin_mult_odd at 4 bits: k mod n is replaced
  // by the odd one of k, n - k (the sign goes to the result); digit w = (nibble w | 1) - 16 where nibble w + 1 is even (its forced low bit is
  // what the 16 pays for), the top digit = nibble 63 | 1: sixty-four odd digits in [-15, 15].  The accumulator starts from the top entry
  // and takes 63 mixed additions; |prefix| < 16^w never meets +-(digit 16^w) and the total stays below n, so no addition is exceptional.
  fe kf = fe_load(k, i);
  fe order;
#pragma unroll
  for (int j = 0; j < 8; ++j) order.w[j] = curve_order<C>::N[j];
  {
    fe d;
    const uint32_t borrow = sub8_3(d, kf, order);        // k < 2^256 < 2n
    kf = fe_select(borrow, kf, d);
  }
  const bool zero = fe_is_zero(kf);
  const uint32_t flip = 0u - (uint32_t)((kf.w[0] & 1u) == 0u);
  {
    fe nk;
    (void)sub8_3(nk, order, kf);
    kf = fe_select(flip, nk, kf);
  }
  const uint32_t zmask = 0u - (uint32_t)zero;
  kf.w[0] = zmask ? 1u : kf.w[0];                        // any odd value; replaced by infinity below
  const uint32_t special = comb_special(kf, reinterpret_cast<const uint4*>(table) + ((size_t)WINDOWS * W4E + 1) * 4);
  comb acc;
  uint32_t above = kf.w[7] >> 28;
  {
    fe tx, ty;
    if constexpr (CT) lds_entry_scan<W4E>(&lds[(63 * W4E) * 4], above >> 1, tx, ty);
    else lds_entry(&lds[((63 * W4E) + (above >> 1)) * 4], tx, ty);
    acc.start(tx, ty, 0u);
  }
  auto digit = [&](uint32_t& mag, uint32_t& neg) {                    // the next nibble down: kf <<= 4 moves it to the top
#pragma unroll
    for (int j = 7; j > 0; --j) kf.w[j] = __builtin_amdgcn_alignbit(kf.w[j], kf.w[j - 1], 28);
    kf.w[0] <<= 4;
    const uint32_t nib = kf.w[7] >> 28;
    const uint32_t u = nib | 1u;
    neg = 0u - (uint32_t)((above & 1u) == 0u);
    mag = neg ? 16u - u : u;
    above = nib;
  };
#pragma unroll 1
  for (int w = 62; w >= 0; --w) {
    uint32_t mag, neg;
    digit(mag, neg);
    fe tx, ty;
    if constexpr (CT) lds_entry_scan<W4E>(&lds[(w * W4E) * 4], mag >> 1, tx, ty);
    else lds_entry(&lds[((w * W4E) + (mag >> 1)) * 4], tx, ty);
    acc.add(tx, ty, neg);
  }
  comb_take_special<CT>(special, reinterpret_cast<const uint4*>(table) + (size_t)WINDOWS * W4E * 4, acc);
  jpoint A = acc.finish();
  A.y = fe_select(flip, fe_neg<CI>(A.y), A.y);
#pragma unroll
  for (int j = 0; j < 8; ++j) { A.x.w[j] &= ~zmask; A.y.w[j] &= ~zmask; A.z.w[j] &= ~zmask; }      // k = 0 mod n: infinity
  fe_store(ox, i, A.x); fe_store(oy, i, A.y); fe_store(oz, i, A.z);
}

// ---- signed WB-bit windows (WB = 5: 51 mixed additions, WB = 7: 36, instead of 63) ---------------
// Odd digits (the kernel below): table entry (i, d) = (2d + 1) * 2^(WB i) * G for d = 0..2^(WB-1) - 1 -- 52 x 16 x 64 B = 53 248 B (WB = 5) or
// 37 x 64 x 64 B = 151 552 B (WB = 7) of LDS.  A negative digit negates the table point's y.  Same affine results as the 4-bit kernel and the ladder.
// (Round 2's carry recoding of unsigned digits was measured against it and removed.)
template <int WB> struct swin {
  static constexpr int WINDOWS = (256 + WB - 1) / WB;        // 52 / 37 odd digits cover 256 bits: no carry window
  static constexpr int ENTRIES = 1 << (WB - 1);
  static constexpr int TABLE_WORDS = WINDOWS * ENTRIES * 16;
};
// One workgroup per CU is all that fits beside the table, so its size IS the occupancy: 256 / 512 / 768 / 1024 threads = 1 / 2 / 3 / 4 waves per
// SIMD read 390 / 450 / 466 / 475 M/s on P-256.  1024 threads cap the kernel at 128 registers: P-256 needs 119 (first window peeled off the loop),
// secp256k1 spills 18 and is still 2.3 % faster than its spill-free 768-thread form (profiles/r03/ab_fixed_base_signed_workgroup_size.txt).
// Reading the next window's entry before the current addition paid at 768 threads (+0.8 %) and loses at 1024 (its 16 live registers spill):
// gone, profiles/r03/ab_fixed_base_lds_prefetch.txt.
#ifndef ECS_SW_BLOCK
#define ECS_SW_BLOCK 1024
#endif
constexpr int SW_BLOCK = ECS_SW_BLOCK;
template <int WB> __global__ void __launch_bounds__(256) k_pack_table_s(const uint64_t* __restrict__ tx, const uint64_t* __restrict__ ty, uint32_t* __restrict__ table) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= swin<WB>::WINDOWS * swin<WB>::ENTRIES + 1) return;      // + the point of k* (comb_special)
  const fe x = comb::pack(classical_to_fast<C>(fe_load(tx, e))), y = comb::pack(classical_to_fast<C>(fe_load(ty, e)));
#pragma unroll
  for (int i = 0; i < 8; ++i) { table[e * 16 + i] = x.w[i]; table[e * 16 + 8 + i] = y.w[i]; }
}
template <int WB, bool CT, int BLK = SW_BLOCK> __global__ void __launch_bounds__(BLK) k_base_windowed_s(const uint64_t* __restrict__ k, const uint32_t* __restrict__ table,
                                                                                uint64_t* __restrict__ ox, uint64_t* __restrict__ oy, uint64_t* __restrict__ oz, size_t n) {
  extern __shared__ uint4 lds_s[];
  {
    const uint4* src = reinterpret_cast<const uint4*>(table);
    for (int r = threadIdx.x; r < swin<WB>::TABLE_WORDS / 4; r += BLK) lds_s[r] = src[r];
  }
  __syncthreads();
  const size_t i = (size_t)blockIdx.x * BLK + threadIdx.x;
  if (i >= n) return;
  // Odd digits (round 3), the scheme of k_base_windowed_g with the table in LDS: the odd one of k mod n, n - k; digit w = ((k >> WB w) mod
  // 2^(WB + 1) | 1) - 2^WB for every window but the top one, whose digit is what remains | 1; the table holds (2d + 1) 2^(WB w) G.  No zero
  // digit: the first entry starts the sum, WINDOWS - 1 mixed additions follow, nothing to skip.  Summed from the bottom: the one scalar whose
  // last addition meets R = T is k* = n - 2 (n mod 2^(WB (WINDOWS - 1))) (comb_special).
  constexpr uint32_t FULL = 1u << WB;
  constexpr int NW = swin<WB>::WINDOWS;
  fe kf = fe_load(k, i);
  fe order;
#pragma unroll
  for (int j = 0; j < 8; ++j) order.w[j] = curve_order<C>::N[j];
  {
    fe d;
    const uint32_t borrow = sub8_3(d, kf, order);
    kf = fe_select(borrow, kf, d);
  }
  const bool zero = fe_is_zero(kf);
  const uint32_t flip = 0u - (uint32_t)((kf.w[0] & 1u) == 0u);
  {
    fe nk;
    (void)sub8_3(nk, order, kf);
    kf = fe_select(flip, nk, kf);
  }
  const uint4* gtab = reinterpret_cast<const uint4*>(table);
  const uint32_t special = comb_special(kf, gtab + ((size_t)NW * swin<WB>::ENTRIES + 1) * 4);
  uint32_t kk[9];
#pragma unroll
  for (int j = 0; j < 8; ++j) kk[j] = kf.w[j];
  kk[8] = 0;
  if (zero) kk[0] = 1;
  comb acc;
  auto digit = [&](int w, uint32_t& mag, uint32_t& neg) {             // window w (wave-uniform), then shift; selects, no branch
    const uint32_t u = (kk[0] & (2u * FULL - 1u)) | 1u;
    const uint32_t sneg = 0u - (uint32_t)(u < FULL);
    const uint32_t smag = sneg ? FULL - u : u - FULL;
    const bool top = w + 1 >= NW;                                       // what remains: the positive top digit
    neg = top ? 0u : sneg;
    mag = top ? (kk[0] | 1u) : smag;
#pragma unroll
    for (int j = 0; j < 8; ++j) kk[j] = __builtin_amdgcn_alignbit(kk[j + 1], kk[j], WB);
  };
  {
    uint32_t mag, neg;
    digit(0, mag, neg);
    fe tx, ty;
    if constexpr (CT) lds_entry_scan<swin<WB>::ENTRIES>(&lds_s[0], mag >> 1, tx, ty);       // ALG_CONSTANT_TIME: all 2^(WB-1) entries, lane masks
    else lds_entry(&lds_s[(size_t)(mag >> 1) * 4], tx, ty);
    acc.start(tx, ty, neg);
  }
#pragma unroll 1
  for (int w = 1; w < NW; ++w) {
    uint32_t mag, neg;
    digit(w, mag, neg);
    fe tx, ty;
    if constexpr (CT) lds_entry_scan<swin<WB>::ENTRIES>(&lds_s[(size_t)w * swin<WB>::ENTRIES * 4], mag >> 1, tx, ty);
    else lds_entry(&lds_s[((size_t)w * swin<WB>::ENTRIES + (mag >> 1)) * 4], tx, ty);
    acc.add(tx, ty, neg);
  }
  comb_take_special<CT>(special, gtab + (size_t)NW * swin<WB>::ENTRIES * 4, acc);
  jpoint A = acc.finish();
  A.y = fe_select(flip, fe_neg<CI>(A.y), A.y);
  if constexpr (CT) {                                                  // k = 0 mod n: infinity, by masks (a branch over 24 moves could skip them)
    const uint32_t keep = 0u - (uint32_t)!zero;
#pragma unroll
    for (int j = 0; j < 8; ++j) { A.x.w[j] &= keep; A.y.w[j] &= keep; A.z.w[j] &= keep; }
  } else if (zero) {
#pragma unroll
    for (int j = 0; j < 8; ++j) { A.x.w[j] = 0; A.y.w[j] = 0; A.z.w[j] = 0; }
  }
  fe_store(ox, i, A.x); fe_store(oy, i, A.y); fe_store(oz, i, A.z);
}

// GW_BITS-bit windows over a table in device memory (20 bits: 13 windows x 524 288 entries x 64 B = 436 MB per curve),
// odd digits only.  k is reduced mod n and replaced by the odd one of k, n - k (the sign goes to the result); then digit i
// = (bits [GW i, GW i + GW] of k with bit GW i forced to 1) - 2^GW for every window but the last, whose digit is what
// remains | 1: 13 odd digits, none zero, the last positive.  The table holds the ODD multiples (2d + 1) 2^(GW i) G.  No
// zero digit: the accumulator starts from the first entry and takes 12 mixed additions, with no "skip" or "infinity"
// selects.  The next window's entry is requested before the current addition so that the HBM latency hides behind
// ~2 300 VALU instructions.
constexpr int GW_BITS = launch::BIG_WINDOW_BITS;
constexpr int GW_WINDOWS = (256 + GW_BITS - 1) / GW_BITS;
constexpr int GW_ENTRIES = 1 << (GW_BITS - 1);
constexpr int GW_BLOCK = 256;
__global__ void __launch_bounds__(256) k_pack_table_n(const uint64_t* __restrict__ tx, const uint64_t* __restrict__ ty, uint32_t* __restrict__ table, size_t count) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= count) return;
  const fe x = comb_big::pack(classical_to_fast<C>(fe_load(tx, e))), y = comb_big::pack(classical_to_fast<C>(fe_load(ty, e)));
#pragma unroll
  for (int i = 0; i < 8; ++i) { table[e * 16 + i] = x.w[i]; table[e * 16 + 8 + i] = y.w[i]; }
}
__global__ void __launch_bounds__(GW_BLOCK) k_base_windowed_g(const uint64_t* __restrict__ k, const uint4* __restrict__ table,
                                                              uint64_t* __restrict__ ox, uint64_t* __restrict__ oy, uint64_t* __restrict__ oz, size_t n) {
  const size_t i = (size_t)blockIdx.x * GW_BLOCK + threadIdx.x;
  if (i >= n) return;
  constexpr uint32_t FULL = 1u << GW_BITS;
  fe kf = fe_load(k, i);
  fe order;
#pragma unroll
  for (int j = 0; j < 8; ++j) order.w[j] = curve_order<C>::N[j];
  {                                                     // k mod n (k < 2^256 < 2n)
    fe d;
    const uint32_t borrow = sub8_3(d, kf, order);
    kf = fe_select(borrow, kf, d);
  }
  const bool zero = fe_is_zero(kf);
  const uint32_t flip = 0u - (uint32_t)((kf.w[0] & 1u) == 0u);     // even: use n - k (odd) and negate the result
  {
    fe nk;
    (void)sub8_3(nk, order, kf);
    kf = fe_select(flip, nk, kf);
  }
  const uint32_t special = comb_special(kf, table + ((size_t)GW_WINDOWS * GW_ENTRIES + 1) * 4);
  uint32_t kk[9];
#pragma unroll
  for (int j = 0; j < 8; ++j) kk[j] = kf.w[j];
  kk[8] = 0;
  if (zero) kk[0] = 1;                                  // any odd value; replaced by infinity below
  auto digit = [&](int w, uint32_t& mag, uint32_t& neg) {             // window w (wave-uniform), then shift
    if (w + 1 < GW_WINDOWS) {
      const uint32_t u = (kk[0] & (2u * FULL - 1u)) | 1u;            // GW_BITS + 1 bits, odd
      neg = 0u - (uint32_t)(u < FULL);
      mag = neg ? FULL - u : u - FULL;
    } else {
      neg = 0u; mag = kk[0] | 1u;                                      // what remains: the positive top digit
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) kk[j] = __builtin_amdgcn_alignbit(kk[j + 1], kk[j], GW_BITS);
    kk[8] = 0;
  };
  auto fetch = [&](int w, uint32_t mag, uint4 (&q)[4]) {
    const uint4* e = table + ((size_t)w * GW_ENTRIES + (mag >> 1)) * 4;     // slot of the odd multiple mag = 2 slot + 1
    q[0] = e[0]; q[1] = e[1]; q[2] = e[2]; q[3] = e[3];
  };
  auto unpack = [](const uint4 (&q)[4], fe& tx, fe& ty) {
    tx.w[0] = q[0].x; tx.w[1] = q[0].y; tx.w[2] = q[0].z; tx.w[3] = q[0].w; tx.w[4] = q[1].x; tx.w[5] = q[1].y; tx.w[6] = q[1].z; tx.w[7] = q[1].w;
    ty.w[0] = q[2].x; ty.w[1] = q[2].y; ty.w[2] = q[2].z; ty.w[3] = q[2].w; ty.w[4] = q[3].x; ty.w[5] = q[3].y; ty.w[6] = q[3].z; ty.w[7] = q[3].w;
  };
  uint32_t mag, neg;
  uint4 q[4];
  digit(0, mag, neg);
  fetch(0, mag, q);
  comb_big acc;
  {
    fe tx, ty;
    unpack(q, tx, ty);
    const uint32_t first_neg = neg;
    digit(1, mag, neg); fetch(1, mag, q);
    acc.start(tx, ty, first_neg);
  }
#pragma unroll 1
  for (int w = 1; w < GW_WINDOWS; ++w) {
    fe tx, ty;
    unpack(q, tx, ty);
    const uint32_t cur_neg = neg;
    if (w + 1 < GW_WINDOWS) { digit(w + 1, mag, neg); fetch(w + 1, mag, q); }       // in flight during this window's addition
    acc.add(tx, ty, cur_neg);
  }
  comb_take_special(special, table + (size_t)GW_WINDOWS * GW_ENTRIES * 4, acc);    // k = +-(n - 2 (n mod 2^240)): R = T at the top window
  jpoint A = acc.finish();
  A.y = fe_select(flip, fe_neg<CI>(A.y), A.y);
  if (zero) {
#pragma unroll
    for (int j = 0; j < 8; ++j) { A.x.w[j] = 0; A.y.w[j] = 0; A.z.w[j] = 0; }
  }
  fe_store(ox, i, A.x); fe_store(oy, i, A.y); fe_store(oz, i, A.z);
}
}  // namespace

namespace launch {
template <> void point_launch<C>::to_affine_batched(hipStream_t s, const uint64_t* jx, const uint64_t* jy, const uint64_t* jz, uint64_t* x, uint64_t* y, size_t n, bool in_fast) {
  // 2^17 lanes keep two waves on every SIMD; beyond that give each lane up to 128 elements (the shared inversion is 267 field
  // multiplications per LANE: at 2^24 points, 128 per lane instead of 32 takes to_affine from 10.9 to 13.5 G points/s; measured
  // with 2^18 and 2^19 lanes as well, tools/ta_sweep.py: slower at every size)
  size_t m = n >> 17; if (m < 1) m = 1; if (m > BATCH_INVERSION_MAX) m = BATCH_INVERSION_MAX;
  const size_t lanes = (n + m - 1) / m;
  const dim3 grid((unsigned)((lanes + 255) / 256));
  if (in_fast) hipLaunchKernelGGL(k_to_affine_batched<true>, grid, dim3(256), 0, s, jx, jy, jz, x, y, n, lanes, (int)m);
  else hipLaunchKernelGGL(k_to_affine_batched<false>, grid, dim3(256), 0, s, jx, jy, jz, x, y, n, lanes, (int)m);
}
template <> void point_launch<C>::x_mod_n_equals(hipStream_t s, const uint64_t* x, const uint8_t* finite, const uint64_t* r, uint8_t* ok, size_t n) {
  hipLaunchKernelGGL(k_x_mod_n_equals, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, x, finite, r, ok, n);
}
template <> void point_launch<C>::inverse_batched(hipStream_t s, const uint64_t* a, uint64_t* out, size_t n) {
  size_t m = n >> 17; if (m < 1) m = 1; if (m > BATCH_INVERSION_MAX) m = BATCH_INVERSION_MAX;
  const size_t lanes = (n + m - 1) / m;
  hipLaunchKernelGGL(k_inverse_batched, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, s, a, out, n, lanes, (int)m);
}
template <> void point_launch<C>::affine_add_batched(hipStream_t s, const uint64_t* ax, const uint64_t* ay, const uint64_t* bx, const uint64_t* by,
                                                     uint64_t* rx, uint64_t* ry, uint8_t* finite, size_t n) {
  size_t m = n >> 17; if (m < 1) m = 1; if (m > BATCH_INVERSION_MAX) m = BATCH_INVERSION_MAX;
  const size_t lanes = (n + m - 1) / m;
  hipLaunchKernelGGL(k_affine_add_batched, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, s, ax, ay, bx, by, rx, ry, finite, n, lanes, (int)m);
}
template <> void point_launch<C>::pack_table(hipStream_t s, const uint64_t* tx, const uint64_t* ty, uint32_t* table) {
  hipLaunchKernelGGL(k_pack_table, dim3(4), dim3(256), 0, s, tx, ty, table);
}
template <int WB, bool CT, int BLK = SW_BLOCK> static void launch_swin(hipStream_t s, const uint64_t* k, const uint32_t* table, uint64_t* ox, uint64_t* oy, uint64_t* oz, size_t n) {
  // 53 / 88 / 152 KB of dynamic LDS: above the 64 KiB default limit from 6 bits on (per device: set on every launch, it is cheap)
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k_base_windowed_s<WB, CT, BLK>), hipFuncAttributeMaxDynamicSharedMemorySize, swin<WB>::TABLE_WORDS * 4);
  hipLaunchKernelGGL((k_base_windowed_s<WB, CT, BLK>), dim3((unsigned)((n + BLK - 1) / BLK)), dim3(BLK), swin<WB>::TABLE_WORDS * 4, s, k, table, ox, oy, oz, n);
}
template <> void point_launch<C>::pack_table_signed(hipStream_t s, int wbits, const uint64_t* tx, const uint64_t* ty, uint32_t* table) {
  if (wbits == 5) hipLaunchKernelGGL(k_pack_table_s<5>, dim3((swin<5>::WINDOWS * swin<5>::ENTRIES + 256) / 256), dim3(256), 0, s, tx, ty, table);
  else hipLaunchKernelGGL(k_pack_table_s<7>, dim3((swin<7>::WINDOWS * swin<7>::ENTRIES + 255) / 256), dim3(256), 0, s, tx, ty, table);
}
template <> void point_launch<C>::base_windowed_signed(hipStream_t s, const uint64_t* k, const uint32_t* table, uint64_t* ox, uint64_t* oy, uint64_t* oz, size_t n, bool constant_time) {
  // the constant-time comb (every entry of a window read): 5-bit windows (53 KB), three 256-thread workgroups per CU; public scalars: 7-bit windows.
  // (6-bit windows, and constant time at 7 bits with its 64 entries to read per window, were measured and removed: capi.hip CT_WBITS.)
  if (constant_time) launch_swin<5, true, 256>(s, k, table, ox, oy, oz, n);
  else launch_swin<7, false>(s, k, table, ox, oy, oz, n);
}
template <> void point_launch<C>::pack_table_big(hipStream_t s, const uint64_t* tx, const uint64_t* ty, uint32_t* table) {
  const size_t count = (size_t)GW_WINDOWS * GW_ENTRIES + 1;        // + the point of k* (comb_special)
  hipLaunchKernelGGL(k_pack_table_n, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, s, tx, ty, table, count);
}
template <> void point_launch<C>::base_windowed_big(hipStream_t s, const uint64_t* k, const uint32_t* table, uint64_t* ox, uint64_t* oy, uint64_t* oz, size_t n) {
  hipLaunchKernelGGL(k_base_windowed_g, dim3((unsigned)((n + GW_BLOCK - 1) / GW_BLOCK)), dim3(GW_BLOCK), 0, s, k, reinterpret_cast<const uint4*>(table), ox, oy, oz, n);
}
template <> void point_launch<C>::base_windowed(hipStream_t s, const uint64_t* k, const uint32_t* table, uint64_t* ox, uint64_t* oy, uint64_t* oz, size_t n, bool constant_time) {
  const dim3 grid((unsigned)((n + WBLOCK - 1) / WBLOCK));
  // (no entry point asks for constant_time since the 5-bit comb replaced this one there; tests/test_constant_time_isa.py still holds k_base_windowed<true> to the ISA)
  if (constant_time) { hipLaunchKernelGGL(k_base_windowed<true>, grid, dim3(WBLOCK), 0, s, k, table, ox, oy, oz, n); return; }
  hipLaunchKernelGGL(k_base_windowed<false>, grid, dim3(WBLOCK), 0, s, k, table, ox, oy, oz, n);
}
}  // namespace launch
}  // namespace ecsimd_hip
