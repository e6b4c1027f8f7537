// k_schnorr_batch.hip -- BIP-340 batch verification (include/ecsimd_schnorr_batch.h): the kernels around the two bucket sums.  PUBLIC data only.
//
// tools/schnorr_batch_model.py is the normative statement; the stages, in the order capi.hip enqueues them:
//   * k_sb_front     one lane per signature: P = the even-y lift of px, R = the even-y lift of r, E = the challenge digest of (r, px, m) in full,
//                    leaf = H_leaf(E || s).  A lane with px or r on no point (or >= p) or s >= n is MALFORMED: it still writes its leaf, counts itself in
//                    head->malformed, and contributes (0, 0) -- the sums' point at infinity -- with valid = 0.
//   * k_sb_node      one level of the fan-16 hash tree: lane j hashes children 16 j .. in lane order (k <= 16 of them: the block loop's trip count is k / 2 + 1).
//   * k_sb_seed      one lane: seed = H_seed(root || n as 8 big-endian bytes).
//   * k_sb_scalars   one lane per signature: a = (low 128 bits of H_a(seed || i)) | 1, a e mod n with e = E mod n, a s mod n; both products 0 on a malformed lane.
//   * k_sb_sum       one level of the fan-16 tree of additions modulo n; the last level's one lane writes n - sum (0 stays 0) and G: term u of the key sum.
//   * k_sb_accept    one lane: ok = no lane malformed, no invalid point in either sum, and the sums cancel.
// node, seed, the randomizer and the sum are batch_tree.cuh's bodies under this call's tags; the per-lane route's reduction is k_msm_common.hip's.
// Every tagged hash starts from the state after its tag block: five compile-time literals (SCHNORR_BATCH_MID, pinned to hashlib by tests/test_schnorr_batch_cpu.py).
#include "kernels.h"
#include "sha256.cuh"
#include "lift.cuh"
#include "batch_tree.cuh"

namespace ecsimd_hip {
namespace {
using launch::BLOCK;
using launch::words8;
using launch::schnorr_batch_head;
#define GID size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x; if (i >= n) return

// The SHA-256 state after the block SHA256(tag) || SHA256(tag), tag = "ecsimd/schnorr-batch/leaf", "ecsimd/schnorr-batch/node", "ecsimd/schnorr-batch/seed",
// "ecsimd/schnorr-batch/a", "BIP0340/challenge"
constexpr int SB_CHALLENGE = 4;                                // (the first four: batch_tree.cuh's order)
struct schnorr_batch_consts {
  static constexpr uint32_t SCHNORR_BATCH_MID[5][8] = {
      {0x7779a7c6u, 0x3456baf4u, 0xf16728a7u, 0x90b4841du, 0x08db76afu, 0x5301c9ffu, 0x2232d730u, 0x1214dca0u},
      {0x1d638488u, 0x0a1de368u, 0x723ddec2u, 0xed28ac0du, 0x0d9ebbb2u, 0xf39d26bdu, 0x58ddd45bu, 0xd764b89au},
      {0xdc917d3du, 0xe712b88au, 0xaa50d908u, 0xbad51688u, 0xd8782f0fu, 0x19146953u, 0xf5861bcdu, 0x169b8603u},
      {0x1f4e0feeu, 0x694b940fu, 0x722b29fdu, 0x6586f4b6u, 0x47ac54cau, 0x59a009c6u, 0x2aa70cbcu, 0xedc4debcu},
      {0x9cecba11u, 0x23925381u, 0x11679112u, 0xd1627e0fu, 0x97c87550u, 0x003cc765u, 0x90f61164u, 0x33e9b66au}};
  ECS_DEV static uint32_t mid(int tag, int j) { return SCHNORR_BATCH_MID[tag][j]; }
};
using TAGS = schnorr_batch_consts;
// int(H_tag(a || b || m)): the tag block's midstate, the block a || b, then the message with the padding of a hash of 128 + bytes bytes -- k_schnorr.hip's
// tagged_hash_2x32, word for word (that unit keeps its own: its kernels' listings are held to instruction counts and its rates are measured)
template <int TAG> ECS_DEV fe tagged_hash_2x32(const fe& a, const fe& b, const uint8_t* __restrict__ m, size_t msg_bytes, uint32_t aligned) {
  sha256_state s = mid<TAGS, TAG>();
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
// H_tag(bytes(a) || bytes(b)): 64 bytes are one block, the padding a block of its own
template <int TAG> ECS_DEV fe hash_2x32(const fe& a, const fe& b) {
  sha256_state s = mid<TAGS, TAG>();
  sha256_block m;
#pragma unroll
  for (int j = 0; j < 8; ++j) { m.w[j] = a.w[7 - j]; m.w[8 + j] = b.w[7 - j]; }
  sha256_compress(s, m);
#pragma unroll
  for (int j = 0; j < 16; ++j) m.w[j] = 0u;
  m.w[0] = 0x80000000u; m.w[15] = (64u + 64u) * 8u;
  sha256_compress(s, m);
  return sha_digest_fe(s);
}
__global__ void __launch_bounds__(BLOCK) k_sb_front(words8 order, const uint64_t* __restrict__ pxv, const uint64_t* __restrict__ rv, const uint64_t* __restrict__ sv,
                                                    const uint8_t* __restrict__ msg, size_t msg_bytes, size_t stride, uint32_t aligned, uint64_t* __restrict__ Ev,
                                                    uint64_t* __restrict__ leafv, uint64_t* __restrict__ Px, uint64_t* __restrict__ Py, uint64_t* __restrict__ Rx,
                                                    uint64_t* __restrict__ Ry, uint8_t* __restrict__ valid, uint32_t* __restrict__ malformed, size_t n) {
  GID;
  constexpr int C = CURVE_SECP256K1;
  const fe N = w8_words(order);
  const fe r = fe_load(rv, i), s = fe_load(sv, i);
  fe px = fe_load(pxv, i), rx = r, py, ry;
  const fe E = tagged_hash_2x32<SB_CHALLENGE>(r, px, msg + i * stride, msg_bytes, aligned);
  fe_store(Ev, i, E);
  fe_store(leafv, i, hash_2x32<BATCH_LEAF>(E, s));
  bool ok = lift_y<C>(px, 0u, py);                             // (false where px >= p)
  ok = lift_y<C>(rx, 0u, ry) && ok;                            // (false where r >= p)
  ok = ok && g_less(s, N);
  if (!ok) { px = fe_zero(); py = fe_zero(); rx = fe_zero(); ry = fe_zero(); atomicAdd(malformed, 1u); }
  fe_store(Px, i, px); fe_store(Py, i, py);
  fe_store(Rx, i, rx); fe_store(Ry, i, ry);
  valid[i] = (uint8_t)ok;
}

__global__ void __launch_bounds__(BLOCK) k_sb_node(const uint64_t* __restrict__ in, size_t count, uint64_t* __restrict__ out, size_t n) {
  GID;
  batch_node<TAGS>(in, count, out, i);
}

__global__ void __launch_bounds__(64) k_sb_seed(const uint64_t* __restrict__ root, uint64_t n, schnorr_batch_head* __restrict__ head) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  batch_seed<TAGS>(root, n, head->seed);
}

__global__ void __launch_bounds__(BLOCK) k_sb_scalars(gmod M, const schnorr_batch_head* __restrict__ head, const uint64_t* __restrict__ Ev, const uint64_t* __restrict__ sv,
                                                      const uint8_t* __restrict__ valid, uint64_t* __restrict__ av, uint64_t* __restrict__ aev,
                                                      uint64_t* __restrict__ asv, size_t n) {
  GID;
  const fe N = g_words(M.p);
  const fe a = batch_randomizer<TAGS>(head->seed, i);
  fe e = reduce_once(fe_load(Ev, i), N), s = fe_load(sv, i);
  if (!valid[i]) { e = fe_zero(); s = fe_zero(); }             // (a malformed lane's s may be >= n: g_mul's operands stay below n)
  const fe aR = batch_randomizer_mgry(a, M);
  fe_store(av, i, a);
  fe_store(aev, i, g_mul(aR, e, M));
  fe_store(asv, i, g_mul(aR, s, M));
}

// out[i] = the sum of in[16 i ..] modulo n.  gx != nullptr: the last level (one lane): out[0] = n - sum, 0 staying 0, and (gx, gy)[0] = G.
__global__ void __launch_bounds__(BLOCK) k_sb_sum(gmod M, const uint64_t* __restrict__ in, size_t count, uint64_t* __restrict__ out, uint64_t* __restrict__ gx,
                                                  uint64_t* __restrict__ gy, size_t n) {
  GID;
  const fe acc = batch_sum(M, in, count, i, gx != nullptr);
  if (gx) { fe_store(gx, 0, FE_CONST(CURVE_SECP256K1, GX)); fe_store(gy, 0, FE_CONST(CURVE_SECP256K1, GY)); }
  fe_store(out, i, acc);
}

__global__ void __launch_bounds__(64) k_sb_accept(const schnorr_batch_head* __restrict__ head, uint8_t* __restrict__ okv) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  bool ok = head->malformed == 0u && head->invalid[0] == 0u && head->invalid[1] == 0u;
  const bool f0 = head->finite[0] != 0, f1 = head->finite[1] != 0;
  if (f0 != f1) ok = false;
  else if (f0) {                                               // -(x, y) = (x, p - y): equal x, and the two y add up to p
    fe ysum = fe_load(head->ry[0], 0);
    const uint32_t carry = add8(ysum, fe_load(head->ry[1], 0));
    ok = ok && fe_eq(fe_load(head->rx[0], 0), fe_load(head->rx[1], 0)) && carry == 0u && fe_eq(ysum, FE_CONST(CURVE_SECP256K1, P));
  }
  okv[0] = (uint8_t)ok;
}
}  // namespace

namespace launch {
static_assert(sizeof(schnorr_batch_head) == 192 && sizeof(schnorr_batch_head) % 16 == 0, "schnorr_batch_head: zeroed 16 bytes per lane");
static uint32_t word_aligned(const uint8_t* msg, size_t stride_bytes) { return ((reinterpret_cast<uintptr_t>(msg) | stride_bytes) & 3u) == 0 ? 1u : 0u; }
static size_t fan_lanes(size_t count) { return (count + BATCH_FAN - 1) / BATCH_FAN; }
void schnorr_batch_front(hipStream_t s, const words8& order, const uint64_t* px, const uint64_t* r, const uint64_t* sg, const uint8_t* msg, size_t msg_bytes, size_t stride_bytes,
                         uint64_t* E, uint64_t* leaf, uint64_t* Px, uint64_t* Py, uint64_t* Rx, uint64_t* Ry, uint8_t* valid, schnorr_batch_head* head, size_t n) {
  hipLaunchKernelGGL(k_sb_front, grid_for(n), dim3(BLOCK), 0, s, order, px, r, sg, msg, msg_bytes, stride_bytes, word_aligned(msg, stride_bytes), E, leaf, Px, Py, Rx, Ry, valid,
                     &head->malformed, n);
}
void schnorr_batch_node(hipStream_t s, const uint64_t* in, size_t count, uint64_t* out) {
  hipLaunchKernelGGL(k_sb_node, grid_for(fan_lanes(count)), dim3(BLOCK), 0, s, in, count, out, fan_lanes(count));
}
void schnorr_batch_seed(hipStream_t s, const uint64_t* root, size_t n, schnorr_batch_head* head) {
  hipLaunchKernelGGL(k_sb_seed, dim3(1), dim3(64), 0, s, root, (uint64_t)n, head);
}
void schnorr_batch_scalars(hipStream_t s, const gmod& order, const schnorr_batch_head* head, const uint64_t* E, const uint64_t* sg, const uint8_t* valid, uint64_t* a, uint64_t* ae,
                           uint64_t* as, size_t n) {
  hipLaunchKernelGGL(k_sb_scalars, grid_for(n), dim3(BLOCK), 0, s, order, head, E, sg, valid, a, ae, as, n);
}
void schnorr_batch_sum(hipStream_t s, const gmod& order, const uint64_t* in, size_t count, uint64_t* out, uint64_t* gx, uint64_t* gy) {
  hipLaunchKernelGGL(k_sb_sum, grid_for(fan_lanes(count)), dim3(BLOCK), 0, s, order, in, count, out, gx, gy, fan_lanes(count));
}
void schnorr_batch_accept(hipStream_t s, const schnorr_batch_head* head, uint8_t* ok) {
  hipLaunchKernelGGL(k_sb_accept, dim3(1), dim3(64), 0, s, head, ok);
}
}  // namespace launch
}  // namespace ecsimd_hip
