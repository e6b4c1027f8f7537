// k_schnorr.hip -- BIP-340 Schnorr signatures on secp256k1: the front and back ends that join the existing window loops, the comb and SHA-256.
//
// A tagged hash SHA256(SHA256(tag) || SHA256(tag) || data) starts from the state after its 64-byte tag block: three compile-time literals (BIP340_MID,
// pinned to hashlib by tests/test_schnorr_cpu.py).  The data of the challenge and of the nonce hash begin with two 32-byte integers, exactly one block,
// so with a 32-byte message either hash is two compressions (the second one padded in registers) and the aux hash one; a message of another length
// goes through sha256.cuh's block loop, uniform in the length.
//
// Verification, PUBLIC data:
//   * k_schnorr_verify_front   e = int(H_challenge(r || px || m)) mod n, u1 = s, u2 = n - e (0 stays 0), P = the even-y lift of px (lift.cuh; G where
//                              there is none, a point the sum's window tables can hold), valid = lift && r < p && s < n, u1 = u2 = 0 where not valid.
//                              No inversion modulo n.  The sum u1 G + u2 P is double_scalar_mult's.
//   * k_schnorr_accept         ok = the sum is finite (which invalid lanes never are) && x(R) == r && y(R) even.
// Signing, SECRET data (d, d', t, the nonce hash, k0, k, both affine products): selects by masks only, no branch, address or lane mask made of them, and
// no declassified bit (tools/ct_check.py check_secret_flow holds the ISA to that).  d G and k0 G come from the constant-time comb between the kernels:
//   * k_schnorr_nonce          d' = d or n - d by the parity of y(d G), t = d' xor H_aux(aux), k0 = int(H_nonce(t || px || m)) mod n; 0 where d is not
//                              in [1, n - 1] (a lane whose k0 is 0 is refused by the next kernel, whichever way it came to be 0).
//   * k_schnorr_finish         k = k0 or n - k0 by the parity of y(k0 G), e from (x(R), px, m), s = k + e d' mod n; r, s and px zeroed under the ok mask.
#include "kernels.h"
#include "sha256.cuh"
#include "lift.cuh"

namespace ecsimd_hip {
namespace {
using launch::BLOCK;
using launch::words8;
#define GID size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x; if (i >= n) return

// The SHA-256 state after the block SHA256(tag) || SHA256(tag), tag = "BIP0340/challenge", "BIP0340/aux", "BIP0340/nonce"
enum { TAG_CHALLENGE = 0, TAG_AUX = 1, TAG_NONCE = 2 };
struct bip340_consts {
  static constexpr uint32_t BIP340_MID[3][8] = {
      {0x9cecba11u, 0x23925381u, 0x11679112u, 0xd1627e0fu, 0x97c87550u, 0x003cc765u, 0x90f61164u, 0x33e9b66au},
      {0x24dd3219u, 0x4eba7e70u, 0xca0fabb9u, 0x0fa3166du, 0x3afbe4b1u, 0x4c44df97u, 0x4aac2739u, 0x249e850au},
      {0x46615b35u, 0xf4bfbff7u, 0x9f8dc671u, 0x83627ab3u, 0x60217180u, 0x57358661u, 0x21a29e54u, 0x68b07b4cu}};
};
template <int TAG> ECS_DEV sha256_state tag_midstate() {
  sha256_state s;
#pragma unroll
  for (int j = 0; j < 8; ++j) s.h[j] = bip340_consts::BIP340_MID[TAG][j];
  return s;
}
// The message as the kernels see it, four arguments each: lane i's bytes at msg + i * stride, the length, and `aligned` (sha256.cuh) -- the same on every lane.
#define MSG_ARGS const uint8_t* __restrict__ msg, size_t msg_bytes, size_t stride, uint32_t aligned

// int(H_tag(a || b || m)): the tag block's midstate, the block a || b, then the message with the padding of a hash of 128 + bytes bytes
template <int TAG> ECS_DEV fe tagged_hash_2x32(const fe& a, const fe& b, const uint8_t* __restrict__ m, size_t msg_bytes, uint32_t aligned) {
  sha256_state s = tag_midstate<TAG>();
  sha256_block blk;
#pragma unroll
  for (int j = 0; j < 8; ++j) { blk.w[j] = a.w[7 - j]; blk.w[8 + j] = b.w[7 - j]; }
  sha256_compress(s, blk);
  sha256_absorb_message(s, m, msg_bytes, aligned, 128);
  return sha_digest_fe(s);
}
// v mod n for v < 2^256 < 2 n: one masked subtraction
ECS_DEV fe reduce_once(const fe& v, const fe& N) {
  fe d;
  const uint32_t below = sub8_3(d, v, N);
  return fe_select(below, v, d);
}
// n - v for 0 < v < n, and 0 for v = 0
ECS_DEV fe negate_mod(const fe& v, const fe& N) {
  fe d;
  (void)sub8_3(d, N, v);
  const uint32_t keep = ~g_zero_mask(v);
#pragma unroll
  for (int q = 0; q < 8; ++q) d.w[q] &= keep;
  return d;
}
// all ones where 1 <= v < n
ECS_DEV uint32_t in_range_mask(const fe& v, const fe& N) {
  fe t;
  return sub8_3(t, v, N) & ~g_zero_mask(v);
}

// ---- verification (public data)
__global__ void __launch_bounds__(BLOCK) k_schnorr_verify_front(words8 order, const uint64_t* __restrict__ pxv, const uint64_t* __restrict__ rv, const uint64_t* __restrict__ sv,
                                                                MSG_ARGS, uint64_t* __restrict__ u1, uint64_t* __restrict__ u2, uint64_t* __restrict__ ox,
                                                                uint64_t* __restrict__ oy, uint8_t* __restrict__ valid, size_t n) {
  GID;
  constexpr int C = CURVE_SECP256K1;
  const fe N = w8_words(order), P = FE_CONST(C, P);
  const fe r = fe_load(rv, i), s = fe_load(sv, i);
  fe x = fe_load(pxv, i), y;
  const fe e = reduce_once(tagged_hash_2x32<TAG_CHALLENGE>(r, x, msg + i * stride, msg_bytes, aligned), N);
  bool ok = lift_y<C>(x, 0u, y);
  ok = ok && g_less(r, P) && g_less(s, N);
  fe a = s, b = negate_mod(e, N);
  if (!ok) { x = FE_CONST(C, GX); y = FE_CONST(C, GY); a = fe_zero(); b = fe_zero(); }
  fe_store(u1, i, a); fe_store(u2, i, b);
  fe_store(ox, i, x); fe_store(oy, i, y);
  valid[i] = (uint8_t)ok;
}
// (x, y) = the sum, (0, 0) and finite = 0 where it is infinite or the lane was not valid (clear_invalid)
__global__ void __launch_bounds__(BLOCK) k_schnorr_accept(const uint64_t* __restrict__ xv, const uint64_t* __restrict__ yv, const uint8_t* __restrict__ finite,
                                                          const uint64_t* __restrict__ rv, uint8_t* __restrict__ okv, size_t n) {
  GID;
  const fe x = fe_load(xv, i), r = fe_load(rv, i);
  const uint32_t y0 = (uint32_t)yv[4 * i];
  okv[i] = (uint8_t)(finite[i] != 0 && fe_eq(x, r) && (y0 & 1u) == 0u);
}

// ---- signing (secret data)
// d' = d where y(d G) is even, n - d where it is odd; yP = that y
ECS_DEV fe even_y_key(const fe& d, const fe& yP, const fe& N) {
  fe neg;
  (void)sub8_3(neg, N, d);
  return fe_select(0u - (yP.w[0] & 1u), neg, d);
}
__global__ void __launch_bounds__(BLOCK) k_schnorr_nonce(words8 order, const uint64_t* __restrict__ dv, const uint64_t* __restrict__ auxv, const uint64_t* __restrict__ pxv,
                                                         const uint64_t* __restrict__ pyv, MSG_ARGS, uint64_t* __restrict__ k0v, size_t n) {
  GID;
  const fe N = w8_words(order);
  const fe d = fe_load(dv, i);
  const uint32_t key_ok = in_range_mask(d, N);
  const fe dd = even_y_key(d, fe_load(pyv, i), N);
  sha256_state a;                                              // H_aux(aux): one compression
  if (auxv) {                                                  // (a null pointer is the call's, not the lane's: 32 zero bytes)
    const fe aux = fe_load(auxv, i);
#pragma unroll
    for (int j = 0; j < 8; ++j) a.h[j] = aux.w[7 - j];
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) a.h[j] = 0u;
  }
  sha256_state h = tag_midstate<TAG_AUX>();
  sha256_compress(h, sha_tail_block32(a, 0x80000000u, 96u));
  fe t = sha_digest_fe(h);
#pragma unroll
  for (int q = 0; q < 8; ++q) t.w[q] ^= dd.w[q];
  fe k0 = reduce_once(tagged_hash_2x32<TAG_NONCE>(t, fe_load(pxv, i), msg + i * stride, msg_bytes, aligned), N);
#pragma unroll
  for (int q = 0; q < 8; ++q) k0.w[q] &= key_ok;
  fe_store(k0v, i, k0);
}
// M = n's gmod.  (xR, yR) = the affine k0 G, (xP, yP) = the affine d G, k0 = 0 where the lane is refused.
__global__ void __launch_bounds__(BLOCK) k_schnorr_finish(gmod M, const uint64_t* __restrict__ dv, const uint64_t* __restrict__ k0v, const uint64_t* __restrict__ xPv,
                                                          const uint64_t* __restrict__ yPv, const uint64_t* __restrict__ xRv, const uint64_t* __restrict__ yRv, MSG_ARGS,
                                                          uint64_t* __restrict__ pxo, uint64_t* __restrict__ ro, uint64_t* __restrict__ so, uint8_t* __restrict__ okv, size_t n) {
  GID;
  const fe N = g_words(M.p);
  fe xR = fe_load(xRv, i), xP = fe_load(xPv, i);
  const fe e = reduce_once(tagged_hash_2x32<TAG_CHALLENGE>(xR, xP, msg + i * stride, msg_bytes, aligned), N);
  const fe k0 = fe_load(k0v, i);
  const uint32_t keep = ~g_zero_mask(k0);                      // d was in range and the nonce is not 0
  const fe dd = reduce_once(even_y_key(fe_load(dv, i), fe_load(yPv, i), N), N);   // (a refused lane's d may be anything: keep g_mul's operand below n)
  fe kneg;
  (void)sub8_3(kneg, N, k0);
  const fe k = fe_select(0u - ((uint32_t)yRv[4 * i] & 1u), kneg, k0);
  const fe ed = g_mul(g_mul(e, dd, M), g_words(M.rsq), M);     // e d' mod n
  fe s = g_add(k, ed, M);
#pragma unroll
  for (int q = 0; q < 8; ++q) { xR.w[q] &= keep; s.w[q] &= keep; xP.w[q] &= keep; }
  fe_store(ro, i, xR); fe_store(so, i, s);
  if (pxo) fe_store(pxo, i, xP);
  okv[i] = (uint8_t)(keep & 1u);
}
}  // namespace

namespace launch {
static uint32_t word_aligned(const uint8_t* msg, size_t stride_bytes) { return ((reinterpret_cast<uintptr_t>(msg) | stride_bytes) & 3u) == 0 ? 1u : 0u; }
void schnorr_verify_front(hipStream_t s, const words8& order, const uint64_t* px, const uint64_t* r, const uint64_t* sg, const uint8_t* msg, size_t msg_bytes, size_t stride_bytes,
                          uint64_t* u1, uint64_t* u2, uint64_t* x, uint64_t* y, uint8_t* valid, size_t n) {
  hipLaunchKernelGGL(k_schnorr_verify_front, grid_for(n), dim3(BLOCK), 0, s, order, px, r, sg, msg, msg_bytes, stride_bytes, word_aligned(msg, stride_bytes), u1, u2, x, y, valid, n);
}
void schnorr_accept(hipStream_t s, const uint64_t* x, const uint64_t* y, const uint8_t* finite, const uint64_t* r, uint8_t* ok, size_t n) {
  hipLaunchKernelGGL(k_schnorr_accept, grid_for(n), dim3(BLOCK), 0, s, x, y, finite, r, ok, n);
}
void schnorr_nonce(hipStream_t s, const words8& order, const uint64_t* d, const uint64_t* aux, const uint64_t* px, const uint64_t* py, const uint8_t* msg, size_t msg_bytes,
                   size_t stride_bytes, uint64_t* k0, size_t n) {
  hipLaunchKernelGGL(k_schnorr_nonce, grid_for(n), dim3(BLOCK), 0, s, order, d, aux, px, py, msg, msg_bytes, stride_bytes, word_aligned(msg, stride_bytes), k0, n);
}
void schnorr_finish(hipStream_t s, const gmod& M, const uint64_t* d, const uint64_t* k0, const uint64_t* xP, const uint64_t* yP, const uint64_t* xR, const uint64_t* yR,
                    const uint8_t* msg, size_t msg_bytes, size_t stride_bytes, uint64_t* px, uint64_t* r, uint64_t* sg, uint8_t* ok, size_t n) {
  hipLaunchKernelGGL(k_schnorr_finish, grid_for(n), dim3(BLOCK), 0, s, M, d, k0, xP, yP, xR, yR, msg, msg_bytes, stride_bytes, word_aligned(msg, stride_bytes), px, r, sg, ok, n);
}
}  // namespace launch
}  // namespace ecsimd_hip
