// batch_tree.cuh -- what the two batch verifications (k_schnorr_batch.hip, BIP-340; k_msm_ed25519.hip, Ed25519) derive their randomizers with, ONCE: the fan-16
// hash tree over the leaves, the seed, the randomizers, and the fan-16 tree of additions modulo the group order.  PUBLIC data only.  tools/schnorr_batch_model.py
// and tools/ed25519_batch_model.py are the normative statements; they differ in the tags alone.
//
// Every tagged hash starts from the SHA-256 state after its tag block SHA256(tag) || SHA256(tag): compile-time literals that stay in the unit (the CPU tests pin
// them to hashlib there).  A unit hands them over as a type T with  ECS_DEV static uint32_t T::mid(int tag, int j)  = word j of that state, the tags in the order
// below; a unit's own tags follow them.
#pragma once
#include "kernels.h"
#include "sha256.cuh"
#include "gfield.cuh"

namespace ecsimd_hip {
enum { BATCH_LEAF = 0, BATCH_NODE = 1, BATCH_SEED = 2, BATCH_A = 3 };
constexpr int FAN = launch::BATCH_FAN;

template <class T, int TAG> ECS_DEV sha256_state mid() {
  sha256_state s;
#pragma unroll
  for (int j = 0; j < 8; ++j) s.h[j] = T::mid(TAG, j);
  return s;
}
// H_tag(bytes(a) || v as 8 big-endian bytes): 40 bytes and the padding in one block.  Digests are held as sha_digest_fe leaves them: the big-endian integer of
// the 32 bytes.
template <class T, int TAG> ECS_DEV fe hash_32_8(const fe& a, uint64_t v) {
  sha256_state s = mid<T, TAG>();
  sha256_block m;
#pragma unroll
  for (int j = 0; j < 8; ++j) m.w[j] = a.w[7 - j];
  m.w[8] = (uint32_t)(v >> 32); m.w[9] = (uint32_t)v; m.w[10] = 0x80000000u;
#pragma unroll
  for (int j = 11; j < 15; ++j) m.w[j] = 0u;
  m.w[15] = (64u + 40u) * 8u;
  sha256_compress(s, m);
  return sha_digest_fe(s);
}
// H_node(c_0 || ... || c_{k-1}), c_j = in[first + j], 1 <= k <= 16: two children per block; the padding's first byte follows the last child -- in the second
// half of the last block where k is odd, at the start of a block of its own where it is even -- and the bit length ends that block.
template <class T> ECS_DEV fe hash_children(const uint64_t* __restrict__ in, size_t first, uint32_t k) {
  sha256_state s = mid<T, BATCH_NODE>();
  const uint32_t blocks = k / 2u + 1u;
#pragma unroll 1
  for (uint32_t b = 0; b < blocks; ++b) {
    sha256_block m;
#pragma unroll
    for (int j = 0; j < 16; ++j) m.w[j] = 0u;
    if (2u * b < k) {
      const fe c = fe_load(in, first + 2u * b);
#pragma unroll
      for (int j = 0; j < 8; ++j) m.w[j] = c.w[7 - j];
    } else m.w[0] = 0x80000000u;                               // 2 b == k
    if (2u * b + 1u < k) {
      const fe c = fe_load(in, first + 2u * b + 1u);
#pragma unroll
      for (int j = 0; j < 8; ++j) m.w[8 + j] = c.w[7 - j];
    } else if (2u * b + 1u == k) m.w[8] = 0x80000000u;
    if (b + 1u == blocks) m.w[15] = (64u + 32u * k) * 8u;
    sha256_compress(s, m);
  }
  return sha_digest_fe(s);
}

// The kernels' bodies; i = the lane, below the launch's lane count.
// One level of the hash tree: out[i] = H_node of children 16 i .. in lane order (k <= 16 of them: the block loop's trip count is k / 2 + 1).
template <class T> ECS_DEV void batch_node(const uint64_t* __restrict__ in, size_t count, uint64_t* __restrict__ out, size_t i) {
  const size_t first = i * FAN, left = count - first;
  fe_store(out, i, hash_children<T>(in, first, left < (size_t)FAN ? (uint32_t)left : (uint32_t)FAN));
}
// seed = H_seed(root || n as 8 big-endian bytes)
template <class T> ECS_DEV void batch_seed(const uint64_t* __restrict__ root, uint64_t n, uint64_t* __restrict__ seed) {
  fe_store(seed, 0, hash_32_8<T, BATCH_SEED>(fe_load(root, 0), n));
}
// lane i's randomizer: (the low 128 bits of H_a(seed || i)) | 1
template <class T> ECS_DEV fe batch_randomizer(const uint64_t* __restrict__ seed, size_t i) {
  fe a = hash_32_8<T, BATCH_A>(fe_load(seed, 0), (uint64_t)i);
#pragma unroll
  for (int q = 4; q < 8; ++q) a.w[q] = 0u;
  a.w[0] |= 1u;
  return a;
}
// a R mod the order: its Montgomery product with a plain value below the order is their plain product
ECS_DEV fe batch_randomizer_mgry(const fe& a, const gmod& M) { return g_mul(a, g_words(M.rsq), M); }
// One level of the tree of additions: the sum of in[16 i ..] modulo the order; negate (the last level's one lane): the order - sum, 0 staying 0.
ECS_DEV fe batch_sum(const gmod& M, const uint64_t* __restrict__ in, size_t count, size_t i, bool negate) {
  const size_t first = i * FAN, left = count - first;
  const uint32_t k = left < (size_t)FAN ? (uint32_t)left : (uint32_t)FAN;
  fe acc = fe_load(in, first);
#pragma unroll 1
  for (uint32_t j = 1; j < k; ++j) acc = g_add(acc, fe_load(in, first + j), M);
  if (negate) {
    fe neg;
    (void)sub8_3(neg, g_words(M.p), acc);
    const uint32_t keep = ~g_zero_mask(acc);
#pragma unroll
    for (int q = 0; q < 8; ++q) acc.w[q] = neg.w[q] & keep;
  }
  return acc;
}
}  // namespace ecsimd_hip
