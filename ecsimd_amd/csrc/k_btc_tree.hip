// k_btc_tree.hip -- Bitcoin's hashes with one length per lane, and the two trees Bitcoin builds of SHA-256: a block's Merkle tree and BIP-341's script tree.
//
// PUBLIC data throughout (transactions, txids, scripts, control blocks): none of these kernels takes a secret, and their loads, loops and branches follow the
// data's lengths, depths and order.  A unit of its own: k_sha256.hip and k_btc.hip each have a test that counts the kernels and instructions of their listing.
//
// One length per lane (sha256.cuh: sha256_absorb_message_lens, ripemd160.cuh: rmd160_absorb_message_lens); lane i hashes min(lens[i], stride) bytes of its row,
// loads no byte at or behind them (a masked-off load reads the lane's own output slot instead) and loops over its own whole blocks:
//   * k_sha256_lens<ALIGNED, MODE>   MODE 0: SHA256(m), 1: SHA256(SHA256(m)) as k_sha256d, 2: RIPEMD160(SHA256(m)) as k_hash160.
//   * k_ripemd160_lens<ALIGNED>      RIPEMD160(m).
// Merkle roots (Bitcoin Core's ComputeMerkleRoot), one launch per level, one lane per parent node of every tree of the chunk:
//   * k_merkle_level                 the lane's tree by bisection over the level's node offsets; parent j = SHA256d(be32(L[2j]) || be32(L[2j + 1])), the last node
//                                    paired with itself where the count is odd (its right neighbour is not loaded: it may be another tree's, or nobody's); a tree
//                                    already down to one node passes it through.  Three compressions: the 64 data bytes, the padding block of a 64-byte message
//                                    -- all constants: its schedule folds at compile time --, sha_tail_block32 from the initial state.  mutated[t] = 1 where a
//                                    REAL pair (2j + 1 < count) holds two equal values (CVE-2012-2459): lanes that see one all store the same byte.
// BIP-341 script paths.  A tagged hash starts from the state after the block SHA256(tag) || SHA256(tag): TAPLEAF_MID and TAPBRANCH_MID, compile-time literals
// pinned to hashlib by tests/test_btc_tree_cpu.py:
//   * k_tapleaf_hash<ALIGNED>        H_TapLeaf(version || compact_size(len) || script).  The 2, 4 or 6 prefix bytes are built in registers and enter as the
//                                    "carry" in front of the first script block; the script is read on ITS OWN word grid (whole blocks in the loop, the tail masked
//                                    as above) and every hashed word is a funnel shift of two neighbours of carry || block by the prefix length -- 0, 2 bytes and
//                                    one word more or less, chosen by selects.  The block's last two words are the next block's carry.  Nothing is staged in memory.
//   * k_taproot_merkle_path<ALIGNED> k = leaf; depth times: k = H_TapBranch(min(k, e) || max(k, e)) with e the next 32 bytes of the lane's path, the order that
//                                    of the 32 bytes (the integers'); two compressions a step from TAPBRANCH_MID, the second the constant padding block of a
//                                    128-byte hash.  The loop runs per lane.  depth > 128: ok = 0 and root = 0.
#include "kernels.h"
#include "ripemd160.cuh"

namespace ecsimd_hip {
namespace {
using launch::BLOCK;
#define GID size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x; if (i >= n) return

// ---- one length per lane
ECS_DEV uint32_t lane_len(const uint32_t* __restrict__ lens, size_t i, size_t stride) {
  const uint32_t len = lens[i];
  return len < stride ? len : (uint32_t)stride;                // never past the lane's own stride
}
enum { LENS_SHA256 = 0, LENS_SHA256D = 1, LENS_HASH160 = 2 };
// msg and out are not __restrict__: a masked-off load reads the output slot
template <bool ALIGNED, int MODE>
__global__ void __launch_bounds__(BLOCK) k_sha256_lens(const uint8_t* msg, size_t stride, const uint32_t* __restrict__ lens, void* out, size_t n) {
  GID;
  const uint8_t* spare = static_cast<const uint8_t*>(out) + (MODE == LENS_HASH160 ? 20 : 32) * i;
  sha256_state s = sha256_iv();
  sha256_absorb_message_lens<ALIGNED>(s, msg + i * stride, lane_len(lens, i, stride), spare);
  if constexpr (MODE == LENS_HASH160) {
    rmd160_store(static_cast<uint32_t*>(out) + 5 * i, rmd160_of_sha256(s));
  } else {
    if constexpr (MODE == LENS_SHA256D) {
      sha256_state d = sha256_iv();
      sha256_compress(d, sha_tail_block32(s, 0x80000000u, 32u));
      s = d;
    }
    fe_store(static_cast<uint64_t*>(out), i, sha_digest_fe(s));
  }
}
template <bool ALIGNED>
__global__ void __launch_bounds__(BLOCK) k_ripemd160_lens(const uint8_t* msg, size_t stride, const uint32_t* __restrict__ lens, uint32_t* out, size_t n) {
  GID;
  rmd160_state s = rmd160_iv();
  rmd160_absorb_message_lens<ALIGNED>(s, msg + i * stride, lane_len(lens, i, stride), reinterpret_cast<const uint8_t*>(out + 5 * i));
  rmd160_store(out + 5 * i, s);
}

// ---- Merkle roots
// off_in / off_out: trees + 1 node offsets of the level read and of the level written (off_out strictly increasing: every tree keeps a node); n = off_out[trees].
// A root leaves as it came: the digest as the integer sha256d writes.
__global__ void __launch_bounds__(BLOCK) k_merkle_level(const uint64_t* __restrict__ in, const uint64_t* __restrict__ off_in, const uint64_t* __restrict__ off_out,
                                                        size_t trees, uint64_t* __restrict__ out, uint8_t* __restrict__ mutated, size_t n) {
  GID;
  size_t lo = 0, hi = trees;                                   // off_out[lo] <= i < off_out[hi]
  while (hi - lo > 1) {
    const size_t mid = lo + (hi - lo) / 2;
    if (off_out[mid] <= i) lo = mid; else hi = mid;
  }
  const size_t j = i - off_out[lo], first = off_in[lo], count = off_in[lo + 1] - first;
  if (count == 1) { fe_store(out, i, fe_load(in, first)); return; }
  const bool pair = 2 * j + 1 < count;
  const fe a = fe_load(in, first + 2 * j), b = fe_load(in, first + 2 * j + (pair ? 1 : 0));
  if (pair && mutated) {
    uint32_t diff = 0;
#pragma unroll
    for (int q = 0; q < 8; ++q) diff |= a.w[q] ^ b.w[q];
    if (diff == 0) mutated[lo] = 1;
  }
  sha256_block m;
#pragma unroll
  for (int q = 0; q < 8; ++q) { m.w[q] = a.w[7 - q]; m.w[8 + q] = b.w[7 - q]; }
  sha256_state s = sha256_iv();
  sha256_compress(s, m);
  m.w[0] = 0x80000000u;                                        // the padding block of a hash of 64 bytes
#pragma unroll
  for (int q = 1; q < 15; ++q) m.w[q] = 0u;
  m.w[15] = 64u * 8u;
  sha256_compress(s, m);
  sha256_state d = sha256_iv();
  sha256_compress(d, sha_tail_block32(s, 0x80000000u, 32u));
  fe_store(out, i, sha_digest_fe(d));
}

// ---- BIP-341 script paths
// The SHA-256 states after the blocks SHA256(tag) || SHA256(tag), tag = "TapLeaf" and tag = "TapBranch"
struct taptree_consts {
  static constexpr uint32_t TAPLEAF_MID[8] = {0x9ce0e4e6u, 0x7c116c39u, 0x38b3caf2u, 0xc30f5089u, 0xd3f3936cu, 0x47636e60u, 0x7db33eeau, 0xddc6f0c9u};
  static constexpr uint32_t TAPBRANCH_MID[8] = {0x23a865a9u, 0xb8a40da7u, 0x977c1e04u, 0xc49e246fu, 0xb5be1376u, 0x9d24c9b7u, 0xb583b5d4u, 0xa8d226d2u};
};

// The block that follows the k carried bytes (k = 2, 4 or 6: the low bytes of c0 || c1) with the first 64 - k bytes of w; then c0 || c1 = w's last two words.
// With E = c0, c1, w[0 .. 15]: word j begins k bytes in front of w[j]: E[j + 1] for k = 4, the halves of E[j + 1], E[j + 2] for k = 2, of E[j], E[j + 1] for 6.
ECS_DEV sha256_block tapleaf_shift(uint32_t& c0, uint32_t& c1, const sha256_block& w, uint32_t k) {
  uint32_t a[17];                                              // E[j] for k = 6, else E[j + 1]
  a[0] = k == 6u ? c0 : c1;
  a[1] = k == 6u ? c1 : w.w[0];
#pragma unroll
  for (int j = 2; j < 17; ++j) a[j] = k == 6u ? w.w[j - 2] : w.w[j - 1];
  sha256_block m;
#pragma unroll
  for (int j = 0; j < 16; ++j) m.w[j] = k == 4u ? a[j] : ((a[j] << 16) | (a[j + 1] >> 16));
  c0 = w.w[14]; c1 = w.w[15];
  return m;
}
template <bool ALIGNED>
__global__ void __launch_bounds__(BLOCK) k_tapleaf_hash(const uint8_t* script, size_t script_bytes, size_t stride, const uint32_t* __restrict__ lens,
                                                        const uint8_t* __restrict__ version, uint32_t version_all, uint64_t* out, size_t n) {
  GID;
  const uint32_t len = lens ? lane_len(lens, i, stride) : (uint32_t)script_bytes;
  const uint32_t ver = version ? version[i] : version_all;
  // version || compact_size(len), right-aligned in c0 || c1
  uint32_t k, c0 = 0, c1;
  if (len < 0xfdu) { k = 2; c1 = (ver << 8) | len; }
  else if (len <= 0xffffu) { k = 4; c1 = (ver << 24) | (0xfdu << 16) | ((len & 0xffu) << 8) | (len >> 8); }
  else { k = 6; c0 = (ver << 8) | 0xfeu; c1 = __builtin_bswap32(len); }
  const uint8_t* p = script + i * stride;
  const uint8_t* spare = reinterpret_cast<const uint8_t*>(out + 4 * i);
  sha256_state s;
#pragma unroll
  for (int j = 0; j < 8; ++j) s.h[j] = taptree_consts::TAPLEAF_MID[j];
  const uint32_t full = len >> 6, rem = len & 63u;
#pragma unroll 1
  for (uint32_t b = 0; b < full; ++b) {                        // the script's whole blocks
    sha256_compress(s, tapleaf_shift(c0, c1, sha256_load_block<ALIGNED>(p), k));
    p += 64;
  }
  // the tail: k + rem bytes (at most 69), 0x80, zeros and the bit length of tag block, prefix and script: one block where k + rem <= 55, else two
  sha256_block w = sha256_load_tail<ALIGNED>(p, rem, spare);
  const uint64_t bits = ((uint64_t)len + 64u + k) * 8u;
  const uint32_t tails = k + rem > 55u ? 2u : 1u;
#pragma unroll 1
  for (uint32_t t = 0; t < tails; ++t) {
    sha256_block m = tapleaf_shift(c0, c1, w, k);
    if (t + 1 == tails) { m.w[14] = (uint32_t)(bits >> 32); m.w[15] = (uint32_t)bits; }
    sha256_compress(s, m);
#pragma unroll
    for (int j = 0; j < 16; ++j) w.w[j] = 0u;
  }
  fe_store(out, i, sha_digest_fe(s));
}

template <bool ALIGNED>
__global__ void __launch_bounds__(BLOCK) k_taproot_merkle_path(const uint64_t* __restrict__ leaf, const uint8_t* __restrict__ path, size_t path_stride,
                                                               const uint8_t* __restrict__ depth, uint32_t depth_all, uint64_t* __restrict__ root,
                                                               uint8_t* __restrict__ okv, size_t n) {
  GID;
  uint32_t d = depth ? depth[i] : depth_all;
  const bool ok = d <= 128u;
  if (!ok) d = 0;
  uint32_t k[8];
  sha_words_of(fe_load(leaf, i), k);
  const uint8_t* p = path + i * path_stride;
#pragma unroll 1
  for (uint32_t j = 0; j < d; ++j) {
    uint32_t e[8];
    if constexpr (ALIGNED) {
      const uint32_t* q = reinterpret_cast<const uint32_t*>(p);
#pragma unroll
      for (int t = 0; t < 8; ++t) e[t] = __builtin_bswap32(q[t]);
    } else {
#pragma unroll
      for (int t = 0; t < 8; ++t) e[t] = ((uint32_t)p[4 * t] << 24) | ((uint32_t)p[4 * t + 1] << 16) | ((uint32_t)p[4 * t + 2] << 8) | (uint32_t)p[4 * t + 3];
    }
    p += 32;
    uint32_t borrow = 0;                                       // of e - k: 1 where e < k, the node goes first
#pragma unroll
    for (int t = 7; t >= 0; --t) {
      const uint64_t df = (uint64_t)e[t] - k[t] - borrow;
      borrow = (uint32_t)(df >> 32) & 1u;
    }
    sha256_block m;
#pragma unroll
    for (int t = 0; t < 8; ++t) { m.w[t] = borrow ? e[t] : k[t]; m.w[8 + t] = borrow ? k[t] : e[t]; }
    sha256_state s;
#pragma unroll
    for (int t = 0; t < 8; ++t) s.h[t] = taptree_consts::TAPBRANCH_MID[t];
    sha256_compress(s, m);
    m.w[0] = 0x80000000u;                                      // the padding block of a hash of 128 bytes
#pragma unroll
    for (int t = 1; t < 15; ++t) m.w[t] = 0u;
    m.w[15] = 128u * 8u;
    sha256_compress(s, m);
#pragma unroll
    for (int t = 0; t < 8; ++t) k[t] = s.h[t];
  }
  fe r;
#pragma unroll
  for (int t = 0; t < 8; ++t) r.w[7 - t] = ok ? k[t] : 0u;
  fe_store(root, i, r);
  okv[i] = (uint8_t)ok;
}

bool word_aligned(const uint8_t* msg, size_t stride_bytes) { return ((reinterpret_cast<uintptr_t>(msg) | stride_bytes) & 3u) == 0; }
template <int MODE> void launch_sha256_lens(hipStream_t s, const uint8_t* msg, size_t stride, const uint32_t* lens, void* out, size_t n) {
  if (word_aligned(msg, stride)) hipLaunchKernelGGL((k_sha256_lens<true, MODE>), launch::grid_for(n), dim3(BLOCK), 0, s, msg, stride, lens, out, n);
  else hipLaunchKernelGGL((k_sha256_lens<false, MODE>), launch::grid_for(n), dim3(BLOCK), 0, s, msg, stride, lens, out, n);
}
}  // namespace

namespace launch {
void sha256_lens(hipStream_t s, const uint8_t* msg, size_t stride_bytes, const uint32_t* lens, uint64_t* e, size_t n) { launch_sha256_lens<LENS_SHA256>(s, msg, stride_bytes, lens, e, n); }
void sha256d_lens(hipStream_t s, const uint8_t* msg, size_t stride_bytes, const uint32_t* lens, uint64_t* e, size_t n) { launch_sha256_lens<LENS_SHA256D>(s, msg, stride_bytes, lens, e, n); }
void hash160_lens(hipStream_t s, const uint8_t* msg, size_t stride_bytes, const uint32_t* lens, uint8_t* out20, size_t n) { launch_sha256_lens<LENS_HASH160>(s, msg, stride_bytes, lens, out20, n); }
void ripemd160_lens(hipStream_t s, const uint8_t* msg, size_t stride_bytes, const uint32_t* lens, uint8_t* out20, size_t n) {
  uint32_t* o = reinterpret_cast<uint32_t*>(out20);
  if (word_aligned(msg, stride_bytes)) hipLaunchKernelGGL(k_ripemd160_lens<true>, grid_for(n), dim3(BLOCK), 0, s, msg, stride_bytes, lens, o, n);
  else hipLaunchKernelGGL(k_ripemd160_lens<false>, grid_for(n), dim3(BLOCK), 0, s, msg, stride_bytes, lens, o, n);
}
void merkle_level(hipStream_t s, const uint64_t* in, const uint64_t* off_in, const uint64_t* off_out, size_t trees, uint64_t* out, uint8_t* mutated, size_t n) {
  hipLaunchKernelGGL(k_merkle_level, grid_for(n), dim3(BLOCK), 0, s, in, off_in, off_out, trees, out, mutated, n);
}
void tapleaf_hash(hipStream_t s, const uint8_t* script, size_t script_bytes, size_t stride_bytes, const uint32_t* lens, const uint8_t* version, uint32_t version_all, uint64_t* e,
                  size_t n) {
  if (word_aligned(script, stride_bytes)) hipLaunchKernelGGL(k_tapleaf_hash<true>, grid_for(n), dim3(BLOCK), 0, s, script, script_bytes, stride_bytes, lens, version, version_all, e, n);
  else hipLaunchKernelGGL(k_tapleaf_hash<false>, grid_for(n), dim3(BLOCK), 0, s, script, script_bytes, stride_bytes, lens, version, version_all, e, n);
}
void taproot_merkle_path(hipStream_t s, const uint64_t* leaf, const uint8_t* path, size_t path_stride_bytes, const uint8_t* depth, uint32_t depth_all, uint64_t* root, uint8_t* ok,
                         size_t n) {
  if (word_aligned(path, path_stride_bytes)) hipLaunchKernelGGL(k_taproot_merkle_path<true>, grid_for(n), dim3(BLOCK), 0, s, leaf, path, path_stride_bytes, depth, depth_all, root, ok, n);
  else hipLaunchKernelGGL(k_taproot_merkle_path<false>, grid_for(n), dim3(BLOCK), 0, s, leaf, path, path_stride_bytes, depth, depth_all, root, ok, n);
}
}  // namespace launch
}  // namespace ecsimd_hip
