// k_btc.hip -- what Bitcoin makes of SHA-256 and secp256k1: RIPEMD-160, HASH160, the double SHA-256, public-key hashes, and BIP-341's Taproot key tweaks.
//
// Hashes, PUBLIC data (messages and public keys; lengths equal across lanes, every branch uniform):
//   * k_ripemd160<ALIGNED>        one message per lane through ripemd160.cuh's absorb function; the 20 digest bytes go to out + 20 i as five word stores.
//   * k_hash160<ALIGNED>          RIPEMD160(SHA256(m)): sha256.cuh's block loop, then the digest straight into one RIPEMD block in registers.
//   * k_sha256d                   SHA256(SHA256(m)): the block loop, then ONE compression of sha_tail_block32 from the initial state.
//   * k_btc_pubkey_hash<COMP>     HASH160 of the SEC1 encoding of (qx, qy): the prefix byte shifts x (and y) by one byte against the word grid, so every block
//                                 word is a funnel shift of two neighbours (as hmac97's).  Compressed: 33 bytes, one SHA-256 compression and one RIPEMD-160
//                                 compression; uncompressed: 65 bytes, two and one.  No validation; nothing but the 20 bytes reaches memory.
// Taproot, secp256k1 only.  A tagged hash starts from the state after the block SHA256("TapTweak") || SHA256("TapTweak"): TAPTWEAK_MID, a compile-time literal
// pinned to hashlib by tests/test_btc_cpu.py.  t = int(H_TapTweak(be32(px)))  (key path only: one compression)  or  int(H_TapTweak(be32(px) || be32(h)))  (two).
// t is NOT reduced: t >= n refuses the lane.
// Public data (the chain of ecsimd_hip_xonly_tweak_add / _taproot_tweak_pubkey: front, the public comb t G, add, the simultaneous inversion, accept):
//   * k_tweak_front<MODE>         (x, y) = the even-y lift of px (lift.cuh), tt = t -- given (MODE 0) or hashed (1, 2); valid = lift && t < n; where not valid
//                                 tt = 0 and (x, y) = G, a point the addition can hold.
//   * k_tweak_add                 J = J + (x, y) with J = t G Jacobian in the fast domain: infinity + P = P (t = 0), P + P by the tangent (t G = P),
//                                 P - P = infinity (Z = 0), madd_hmv otherwise.  The branches are on public values.
//   * k_tweak_accept              ok = valid && Z != 0; qx = x(Q), parity = y(Q) & 1, zeros where ok = 0.
// SECRET data (d, d', the affine d G, d_out; t is as secret as x(d G) until px is returned): selects by masks only, no branch, address or lane mask in force at
// a memory access made of them, and no declassified bit (tools/ct_check.py check_secret_flow holds the ISA to that).  d G comes from the constant-time comb and
// the select-only simultaneous inversion in front of this kernel:
//   * k_taproot_seckey<HAS_ROOT>  d' = d or n - d by the parity of y(d G), t from x(d G) (and h), d_out = d' + t mod n; ok = 0 and d_out = px = 0 where d is not
//                                 in [1, n - 1], t >= n or the sum is 0.
#include "kernels.h"
#include "ripemd160.cuh"
#include "lift.cuh"

namespace ecsimd_hip {
namespace {
using launch::BLOCK;
using launch::words8;
#define GID size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x; if (i >= n) return

// ---- the hashes
template <bool ALIGNED>
__global__ void __launch_bounds__(BLOCK) k_ripemd160(const uint8_t* __restrict__ msg, size_t msg_bytes, size_t stride, uint32_t* __restrict__ out, size_t n) {
  GID;
  rmd160_state s = rmd160_iv();
  rmd160_absorb_message<ALIGNED>(s, msg + i * stride, msg_bytes);
  rmd160_store(out + 5 * i, s);
}
__global__ void __launch_bounds__(BLOCK) k_hash160(const uint8_t* __restrict__ msg, size_t msg_bytes, size_t stride, uint32_t* __restrict__ out, size_t n, uint32_t aligned) {
  GID;
  sha256_state s = sha256_iv();
  sha256_absorb_message(s, msg + i * stride, msg_bytes, aligned, 0);
  rmd160_store(out + 5 * i, rmd160_of_sha256(s));
}
__global__ void __launch_bounds__(BLOCK) k_sha256d(const uint8_t* __restrict__ msg, size_t msg_bytes, size_t stride, uint64_t* __restrict__ out, size_t n, uint32_t aligned) {
  GID;
  sha256_state s = sha256_iv();
  sha256_absorb_message(s, msg + i * stride, msg_bytes, aligned, 0);
  sha256_state d = sha256_iv();
  sha256_compress(d, sha_tail_block32(s, 0x80000000u, 32u));
  fe_store(out, i, sha_digest_fe(d));
}
// COMPRESSED: (02 | parity of y) || be32(x); else 04 || be32(x) || be32(y)
template <bool COMPRESSED>
__global__ void __launch_bounds__(BLOCK) k_btc_pubkey_hash(const uint64_t* __restrict__ qx, const uint64_t* __restrict__ qy, uint32_t* __restrict__ out, size_t n) {
  GID;
  auto join = [](uint32_t hi, uint32_t lo) { return (hi << 24) | (lo >> 8); };
  uint32_t x[8];
  sha_words_of(fe_load(qx, i), x);
  sha256_state s = sha256_iv();
  sha256_block a;
  if constexpr (COMPRESSED) {
    const uint32_t prefix = 2u | ((uint32_t)qy[4 * i] & 1u);
    a.w[0] = join(prefix, x[0]);
#pragma unroll
    for (int j = 1; j < 8; ++j) a.w[j] = join(x[j - 1], x[j]);
    a.w[8] = (x[7] << 24) | 0x00800000u;
#pragma unroll
    for (int j = 9; j < 15; ++j) a.w[j] = 0u;
    a.w[15] = 33u * 8u;
    sha256_compress(s, a);
  } else {
    uint32_t y[8];
    sha_words_of(fe_load(qy, i), y);
    a.w[0] = join(4u, x[0]);
#pragma unroll
    for (int j = 1; j < 8; ++j) a.w[j] = join(x[j - 1], x[j]);
    a.w[8] = join(x[7], y[0]);
#pragma unroll
    for (int j = 1; j < 8; ++j) a.w[8 + j] = join(y[j - 1], y[j]);
    sha256_compress(s, a);
    sha256_block b;
    b.w[0] = (y[7] << 24) | 0x00800000u;
#pragma unroll
    for (int j = 1; j < 15; ++j) b.w[j] = 0u;
    b.w[15] = 65u * 8u;
    sha256_compress(s, b);
  }
  rmd160_store(out + 5 * i, rmd160_of_sha256(s));
}

// ---- BIP-341
// The SHA-256 state after the block SHA256(tag) || SHA256(tag), tag = "TapTweak"
struct taproot_consts {
  static constexpr uint32_t TAPTWEAK_MID[8] = {0xd129a2f3u, 0x701c655du, 0x6583b6c3u, 0xb9419727u, 0x95f4e232u, 0x94fd54f4u, 0xa2ae8d85u, 0x47ca590bu};
};
// int(H_TapTweak(be32(px)))  or, HAS_ROOT,  int(H_TapTweak(be32(px) || be32(h)))
template <bool HAS_ROOT> ECS_DEV fe tap_tweak(const fe& px, const fe& h) {
  sha256_state s;
#pragma unroll
  for (int j = 0; j < 8; ++j) s.h[j] = taproot_consts::TAPTWEAK_MID[j];
  sha256_state key;
#pragma unroll
  for (int j = 0; j < 8; ++j) key.h[j] = px.w[7 - j];
  if constexpr (!HAS_ROOT) {
    sha256_compress(s, sha_tail_block32(key, 0x80000000u, 96u));
  } else {
    sha256_block blk;
#pragma unroll
    for (int j = 0; j < 8; ++j) { blk.w[j] = key.h[j]; blk.w[8 + j] = h.w[7 - j]; }
    sha256_compress(s, blk);
    blk.w[0] = 0x80000000u;                                    // the padding block of a hash of 128 bytes
#pragma unroll
    for (int j = 1; j < 15; ++j) blk.w[j] = 0u;
    blk.w[15] = 128u * 8u;
    sha256_compress(s, blk);
  }
  return sha_digest_fe(s);
}

// MODE: launch::tweak_mode.  tv = the tweaks (MODE 0) or the merkle roots (MODE 2); unused in MODE 1.
template <int MODE>
__global__ void __launch_bounds__(BLOCK) k_tweak_front(words8 order, const uint64_t* __restrict__ pxv, const uint64_t* __restrict__ tv, uint64_t* __restrict__ ox,
                                                       uint64_t* __restrict__ oy, uint64_t* __restrict__ ot, uint8_t* __restrict__ valid, size_t n) {
  GID;
  constexpr int C = CURVE_SECP256K1;
  const fe N = w8_words(order);
  fe x = fe_load(pxv, i), y, t;
  if constexpr (MODE == launch::TWEAK_GIVEN) t = fe_load(tv, i);
  else if constexpr (MODE == launch::TWEAK_KEY_PATH) t = tap_tweak<false>(x, x);
  else t = tap_tweak<true>(x, fe_load(tv, i));
  bool ok = lift_y<C>(x, 0u, y);
  ok = ok && g_less(t, N);
  if (!ok) { x = FE_CONST(C, GX); y = FE_CONST(C, GY); t = fe_zero(); }
  fe_store(ox, i, x); fe_store(oy, i, y); fe_store(ot, i, t);
  valid[i] = (uint8_t)ok;
}

// J (Jacobian, fast domain, Z = 0: infinity) += (x, y) (classical affine, a point of the curve).  In place: an element is read and written by its own lane only.
__global__ void __launch_bounds__(BLOCK) k_tweak_add(uint64_t* jx, uint64_t* jy, uint64_t* jz, const uint64_t* __restrict__ xv, const uint64_t* __restrict__ yv, size_t n) {
  GID;
  constexpr int C = CURVE_SECP256K1, CI = curve_domain<C>::fast;
  const fe X1 = fe_load(jx, i), Y1 = fe_load(jy, i), Z1 = fe_load(jz, i);
  const fe x2 = classical_to_fast<C>(fe_load(xv, i)), y2 = classical_to_fast<C>(fe_load(yv, i));
  jpoint R;
  if (g_is_zero(Z1)) {                                         // t = 0: Q = P
    R.x = x2; R.y = y2; R.z = FE_CONST(CI, R_P);
  } else {
    const fe Z1Z1 = fe_sqr<CI>(Z1);
    const fe H = fe_sub<CI>(fe_mul<CI>(x2, Z1Z1), X1), r = fe_sub<CI>(fe_mul<CI>(y2, fe_mul<CI>(Z1Z1, Z1)), Y1);
    if (!g_is_zero(H)) R = madd_hmv<CI>(X1, Y1, Z1, x2, y2);
    else if (g_is_zero(r)) {                                   // t G = P: the tangent at the affine P (a = 0; y != 0 on a curve of odd order)
      const fe yy = fe_sqr<CI>(y2), xx = fe_sqr<CI>(x2);
      const fe S = fe_shl<CI, 2>(fe_mul<CI>(x2, yy)), M = fe_add<CI>(fe_dbl<CI>(xx), xx);
      R.x = fe_sub<CI>(fe_sqr<CI>(M), fe_dbl<CI>(S));
      R.y = fe_sub<CI>(fe_mul<CI>(M, fe_sub<CI>(S, R.x)), fe_shl<CI, 3>(fe_sqr<CI>(yy)));
      R.z = fe_dbl<CI>(y2);
    } else {                                                   // t G = -P: infinity
      R.x = fe_zero(); R.y = fe_zero(); R.z = fe_zero();
    }
  }
  fe_store(jx, i, R.x); fe_store(jy, i, R.y); fe_store(jz, i, R.z);
}

// (ax, ay) = the affine sum ((0, 0) where Z = 0), jz = its Z
__global__ void __launch_bounds__(BLOCK) k_tweak_accept(const uint64_t* __restrict__ ax, const uint64_t* __restrict__ ay, const uint64_t* __restrict__ jz,
                                                        const uint8_t* __restrict__ valid, uint64_t* __restrict__ qx, uint8_t* __restrict__ parity, uint8_t* __restrict__ okv,
                                                        size_t n) {
  GID;
  const bool ok = valid[i] != 0 && !g_is_zero(fe_load(jz, i));
  fe x = fe_load(ax, i);
  if (!ok) x = fe_zero();
  fe_store(qx, i, x);
  parity[i] = (uint8_t)(ok ? ((uint32_t)ay[4 * i] & 1u) : 0u);
  okv[i] = (uint8_t)ok;
}

// ---- the secret key's tweak (secret data: selects only)
// v mod n for v < 2^256 < 2 n: one masked subtraction
ECS_DEV fe reduce_once(const fe& v, const fe& N) {
  fe d;
  const uint32_t below = sub8_3(d, v, N);
  return fe_select(below, v, d);
}
// M = n's gmod.  (xP, yP) = the affine d G.
template <bool HAS_ROOT>
__global__ void __launch_bounds__(BLOCK) k_taproot_seckey(gmod M, const uint64_t* __restrict__ dv, const uint64_t* __restrict__ hv, const uint64_t* __restrict__ xPv,
                                                          const uint64_t* __restrict__ yPv, uint64_t* __restrict__ dout, uint64_t* __restrict__ pxo, uint8_t* __restrict__ okv,
                                                          size_t n) {
  GID;
  const fe N = g_words(M.p);
  const fe d = fe_load(dv, i);
  fe scratch, neg;
  const uint32_t key_ok = sub8_3(scratch, d, N) & ~g_zero_mask(d);                 // all ones where 1 <= d < n
  (void)sub8_3(neg, N, d);
  const fe dd = reduce_once(fe_select(0u - ((uint32_t)yPv[4 * i] & 1u), neg, d), N);   // d or n - d by the parity of y(d G) (a refused lane's d may be anything: below n for g_add)
  fe xP = fe_load(xPv, i);
  fe h = xP;
  if constexpr (HAS_ROOT) h = fe_load(hv, i);
  fe t = tap_tweak<HAS_ROOT>(xP, h);
  const uint32_t t_ok = sub8_3(scratch, t, N);                                     // all ones where t < n
#pragma unroll
  for (int q = 0; q < 8; ++q) t.w[q] &= t_ok;
  fe sum = g_add(dd, t, M);
  const uint32_t keep = key_ok & t_ok & ~g_zero_mask(sum);
#pragma unroll
  for (int q = 0; q < 8; ++q) { sum.w[q] &= keep; xP.w[q] &= keep; }
  fe_store(dout, i, sum);
  if (pxo) fe_store(pxo, i, xP);
  okv[i] = (uint8_t)(keep & 1u);
}
}  // namespace

namespace launch {
static bool word_aligned(const uint8_t* msg, size_t stride_bytes) { return ((reinterpret_cast<uintptr_t>(msg) | stride_bytes) & 3u) == 0; }
void ripemd160(hipStream_t s, const uint8_t* msg, size_t msg_bytes, size_t stride_bytes, uint8_t* out20, size_t n) {
  uint32_t* o = reinterpret_cast<uint32_t*>(out20);
  if (word_aligned(msg, stride_bytes)) hipLaunchKernelGGL(k_ripemd160<true>, grid_for(n), dim3(BLOCK), 0, s, msg, msg_bytes, stride_bytes, o, n);
  else hipLaunchKernelGGL(k_ripemd160<false>, grid_for(n), dim3(BLOCK), 0, s, msg, msg_bytes, stride_bytes, o, n);
}
void hash160(hipStream_t s, const uint8_t* msg, size_t msg_bytes, size_t stride_bytes, uint8_t* out20, size_t n) {
  hipLaunchKernelGGL(k_hash160, grid_for(n), dim3(BLOCK), 0, s, msg, msg_bytes, stride_bytes, reinterpret_cast<uint32_t*>(out20), n, word_aligned(msg, stride_bytes) ? 1u : 0u);
}
void sha256d(hipStream_t s, const uint8_t* msg, size_t msg_bytes, size_t stride_bytes, uint64_t* e, size_t n) {
  hipLaunchKernelGGL(k_sha256d, grid_for(n), dim3(BLOCK), 0, s, msg, msg_bytes, stride_bytes, e, n, word_aligned(msg, stride_bytes) ? 1u : 0u);
}
void btc_pubkey_hash(hipStream_t s, const uint64_t* qx, const uint64_t* qy, uint8_t* out20, size_t n, bool compressed) {
  uint32_t* o = reinterpret_cast<uint32_t*>(out20);
  if (compressed) hipLaunchKernelGGL(k_btc_pubkey_hash<true>, grid_for(n), dim3(BLOCK), 0, s, qx, qy, o, n);
  else hipLaunchKernelGGL(k_btc_pubkey_hash<false>, grid_for(n), dim3(BLOCK), 0, s, qx, qy, o, n);
}
void tweak_front(hipStream_t s, const words8& order, int mode, const uint64_t* px, const uint64_t* t_or_merkle, uint64_t* x, uint64_t* y, uint64_t* tt, uint8_t* valid, size_t n) {
  if (mode == TWEAK_GIVEN) hipLaunchKernelGGL(k_tweak_front<TWEAK_GIVEN>, grid_for(n), dim3(BLOCK), 0, s, order, px, t_or_merkle, x, y, tt, valid, n);
  else if (mode == TWEAK_KEY_PATH) hipLaunchKernelGGL(k_tweak_front<TWEAK_KEY_PATH>, grid_for(n), dim3(BLOCK), 0, s, order, px, t_or_merkle, x, y, tt, valid, n);
  else hipLaunchKernelGGL(k_tweak_front<TWEAK_MERKLE_ROOT>, grid_for(n), dim3(BLOCK), 0, s, order, px, t_or_merkle, x, y, tt, valid, n);
}
void tweak_add(hipStream_t s, uint64_t* jx, uint64_t* jy, uint64_t* jz, const uint64_t* x, const uint64_t* y, size_t n) {
  hipLaunchKernelGGL(k_tweak_add, grid_for(n), dim3(BLOCK), 0, s, jx, jy, jz, x, y, n);
}
void tweak_accept(hipStream_t s, const uint64_t* ax, const uint64_t* ay, const uint64_t* jz, const uint8_t* valid, uint64_t* qx, uint8_t* parity, uint8_t* ok, size_t n) {
  hipLaunchKernelGGL(k_tweak_accept, grid_for(n), dim3(BLOCK), 0, s, ax, ay, jz, valid, qx, parity, ok, n);
}
void taproot_seckey(hipStream_t s, const gmod& M, const uint64_t* d, const uint64_t* merkle, const uint64_t* xP, const uint64_t* yP, uint64_t* d_out, uint64_t* px, uint8_t* ok,
                    size_t n) {
  if (merkle) hipLaunchKernelGGL(k_taproot_seckey<true>, grid_for(n), dim3(BLOCK), 0, s, M, d, merkle, xP, yP, d_out, px, ok, n);
  else hipLaunchKernelGGL(k_taproot_seckey<false>, grid_for(n), dim3(BLOCK), 0, s, M, d, merkle, xP, yP, d_out, px, ok, n);
}
}  // namespace launch
}  // namespace ecsimd_hip
