// k_msm_ed25519.hip -- the bucket method on the twisted Edwards curve, and Ed25519 batch verification on top of it: the kernels behind ecsimd_ed25519_msm,
// ecsimd_ed25519_verify_cofactored, ecsimd_ed25519_verify_batch and ecsimd_ed25519_batch_randomizers (include/ecsimd_ed25519_batch.h).  PUBLIC data only: bucket
// addresses are scalar digits and the verification loop is indexed by them.  tools/ed25519_batch_model.py is the normative statement.
//
// THE SUM.  msm_stages.cuh has the stages and their bodies, k_msm_common.hip the kernels without a curve (zero, scan, scatter); this file gives the stages the
// extended Edwards group on ed25519.cuh's arithmetic (ed_add_precomp 7 M into an ed_point, ed_add 9 M, ed_dbl) and keeps what is the curve's:
//   k_edm_digits    one lane per term: the encoding decoded ONCE (ed_decode, strict; a refused one is counted and contributes nothing: scalar 0), stored as
//                   ed_precomp (y + x, y - x, 2 d x y), the scalar masked to `bits` bits, the histogram of its c-bit digits.
//   k_edm_final     one lane: Horner over the windows; then either the encoding (one inversion) or the extended point as it is (the batch's accept kernel adds two
//                   of them and needs no inversion); the flag and the invalid count.
// Accumulators, buckets, slots and the tree are ed_point, FOUR planes of `total` elements (X at e, Y at total + e, Z at 2 total + e, T at 3 total + e); the identity
// is (0, 1, 1, 0).  The unified addition is complete: NO kernel here branches on the group law -- P + P, P + (-P) and P + identity are the same instructions.
//
// THE BATCH (the order capi.hip enqueues them):
//   k_edb_front     one lane per signature: D = SHA-512(R || A || M) in full, h = D mod L, leaf = H_leaf(D || s), A and R copied into the sums' term arrays; a lane
//                   with s >= L (or a small-order A or R, with the flag) counts itself in head->malformed.  Decoding is the sums' (k_edm_digits counts what it refuses).
//   k_edb_node / k_edb_seed / k_edb_scalars / k_edb_sum   batch_tree.cuh's scaffold under this call's tags and modulo L: the fan-16 hash tree, the seed, z and
//                   z h, z s, the fan-16 tree of additions whose last lane writes L - sum and B's encoding: term n of the key sum.
//   k_edb_accept    one lane: ok = no lane malformed, nothing refused or broken in either sum, and [8](sum 0 + sum 1) is the identity (X = 0 and Y = Z).
// THE PER-LANE RULE: k_edc_front (s < L, A and R decode, h, the table of 1 .. 8 times -A, R's coordinates) and k_edc_loop (ed_straus_vartime, - R, three
// doublings, X = 0 and Y = Z).  The LANES route of the batch is these two into a byte array, then k_msm_common.hip's reduction kernel.
// Every tagged hash starts from the state after its tag block: four compile-time literals (ED25519_BATCH_MID, pinned to hashlib by tests/test_ed25519_batch_cpu.py).
//
// Registers and scratch (build/csrc/k_msm_ed25519-hip-amdgcn-amd-amdhsa-gfx950.s; profiles/r17/ed25519_batch_listing.json): 256-thread workgroups, no kernel spills.
// VGPRs / scratch bytes:  k_edm_digits 152 / 0, k_edm_slices 110 / 0, k_edm_combine 132 / 0, k_edm_chunks 228 / 0, k_edm_tree 124 / 0, k_edm_final 130 / 0,
// k_edb_front 130 / 0, k_edb_node 63 / 0, k_edb_seed 59 / 0, k_edb_scalars 76 / 0, k_edb_sum 38 / 0, k_edb_accept 102 / 0, k_edc_front 230 / 0, k_edc_loop 142 / 0.
// Of the 512 VGPRs a SIMD gives a lane: 4 waves per SIMD for the kernels around one addition (slices, tree: 110 - 124), 3 for those that decode (digits) or
// hold two points across one (combine, final, the verification loop), 2 for k_edm_chunks (run, tot and the multiple) and k_edc_front (two decoded points).
#include "kernels.h"
#include "sha256.cuh"
#include "sha512.cuh"
#include "ed25519.cuh"
#include "msm_stages.cuh"
#include "batch_tree.cuh"

namespace ecsimd_hip {
namespace {
using launch::BLOCK;
using launch::ed25519_batch_head;
#define GID size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x; if (i >= n) return
#define MSG_ARGS const uint8_t* __restrict__ msg, size_t msg_bytes, size_t stride, const uint32_t* __restrict__ lens, uint32_t aligned
#define MSG_PASS msg, msg_bytes, stride, lens, aligned

// ---- four-plane and three-plane arrays
ECS_DEV ed_point edp_load(const uint64_t* __restrict__ a, size_t total, size_t e) {
  return {fe_load(a, e), fe_load(a, total + e), fe_load(a, 2 * total + e), fe_load(a, 3 * total + e)};
}
ECS_DEV void edp_store(uint64_t* __restrict__ a, size_t total, size_t e, const ed_point& p) {
  fe_store(a, e, p.X); fe_store(a, total + e, p.Y); fe_store(a, 2 * total + e, p.Z); fe_store(a, 3 * total + e, p.T);
}
ECS_DEV ed_precomp edq_load(const uint64_t* __restrict__ a, size_t total, size_t e) { return {fe_load(a, e), fe_load(a, total + e), fe_load(a, 2 * total + e)}; }
// all ones where p is the identity: X = 0 and Y = Z (Z is never 0 on this curve)
ECS_DEV uint32_t ed_identity_mask(const ed_point& p) { return fe25519_zero_mask(p.X) & fe25519_eq_mask(p.Y, p.Z); }

// msm_stages.cuh's group: extended accumulators, FOUR planes, the identity (0, 1, 1, 0); the terms are the three planes of ed_precomp k_edm_digits left at pre
struct edwards_group {
  using point = ed_point;
  struct terms { const uint64_t* __restrict__ pre; };
  ECS_DEV static point identity() { return ed_identity(); }
  ECS_DEV static point add(const point& P, const point& Q) { return ed_add(P, Q); }
  ECS_DEV static point dbl(const point& P) { return ed_dbl(P); }
  ECS_DEV static point add_term(const point& P, const terms& t, size_t n, size_t idx) { return ed_add_precomp(P, edq_load(t.pre, n, idx)); }
  ECS_DEV static point load(const uint64_t* __restrict__ a, size_t total, size_t e) { return edp_load(a, total, e); }
  ECS_DEV static void store(uint64_t* __restrict__ a, size_t total, size_t e, const point& P) { edp_store(a, total, e, P); }
};
using G = edwards_group;

// ---- the sum
__global__ void __launch_bounds__(BLOCK) k_edm_digits(const uint8_t* __restrict__ k, uint32_t k_aligned, const uint8_t* __restrict__ pts, uint32_t p_aligned,
                                                      uint64_t* __restrict__ kk, uint64_t* __restrict__ pre, uint32_t* __restrict__ hist, uint32_t* __restrict__ counter,
                                                      size_t n, int bits, int c, int windows) {
  GID;
  ed_point P;
  const uint32_t ok = ed_decode(P, ed_load32(pts + 32 * i, p_aligned));
  if (!ok) atomicAdd(counter, 1u);
  fe kv = mask_bits(ed_load32(k + 32 * i, k_aligned), bits);
  const fe one = fe25519_small(1u);
#pragma unroll
  for (int j = 0; j < 8; ++j) kv.w[j] &= ok;
  fe_store(kk, i, kv);
  fe_store(pre, i, fe25519_select(ok, fe25519_add(P.Y, P.X), one));                       // (a refused term: the identity's entry; its scalar is 0 and no lane adds it)
  fe_store(pre, n + i, fe25519_select(ok, fe25519_sub(P.Y, P.X), one));
  fe_store(pre, 2 * n + i, fe25519_select(ok, fe25519_mul(P.T, fe25519_const<ed25519_consts::D2>()), fe25519_small(0u)));
  msm_histogram(kv, hist, c, windows);
}

__global__ void __launch_bounds__(BLOCK) k_edm_slices(const uint32_t* __restrict__ sorted, const uint64_t* __restrict__ kk, const uint64_t* __restrict__ pre,
                                                      const uint32_t* __restrict__ start, uint64_t* __restrict__ buckets, uint64_t* __restrict__ partial,
                                                      uint32_t* __restrict__ broken, size_t n, size_t T, size_t L, size_t slices, int c, size_t K) {
  msm_slices<G>(sorted, kk, {pre}, start, buckets, partial, broken, n, T, L, slices, c, K);
}
__global__ void __launch_bounds__(BLOCK) k_edm_combine(const uint32_t* __restrict__ start, uint64_t* __restrict__ buckets, const uint64_t* __restrict__ partial,
                                                       uint32_t* __restrict__ broken, size_t L, size_t slices, int c, size_t K) {
  msm_combine<G>(start, buckets, partial, broken, L, slices, c, K);
}
__global__ void __launch_bounds__(BLOCK) k_edm_chunks(const uint64_t* __restrict__ buckets, uint64_t* __restrict__ out, size_t lanes, size_t per_window, int c, int m, size_t K) {
  msm_chunks<G>(buckets, out, lanes, per_window, c, m, K);
}
__global__ void __launch_bounds__(BLOCK) k_edm_tree(uint64_t* arr, size_t total, size_t count, size_t stride, size_t lanes, int fan) {
  msm_tree<G>(arr, total, count, stride, lanes, fan);
}

// One lane: msm_horner, then the result.  raw != nullptr: the extended point (X, Y, Z, T: 16 words of 64 bits) goes there and nothing is encoded; else out = the 32-byte encoding.
__global__ void __launch_bounds__(64) k_edm_final(const uint64_t* __restrict__ arr, size_t total, size_t stride, int windows, int c, const uint32_t* __restrict__ counter,
                                                  uint8_t* __restrict__ out, uint32_t out_aligned, uint64_t* __restrict__ raw, uint8_t* __restrict__ finite,
                                                  uint32_t* __restrict__ invalid) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  ed_point acc = msm_horner<G>(arr, total, stride, windows, c);
  uint32_t bad = counter ? counter[0] : 0u;
  const bool broken = counter && counter[1] != 0u;                      // a broken invariant of the sort: no sum is better than a wrong one (INTERNAL CHECK in the header)
  if (broken) bad = 0xffffffffu;
  const bool fin = !ed_identity_mask(acc);
  if (raw) {
    if (broken) acc = {fe25519_small(1u), fe25519_small(0u), fe25519_small(1u), fe25519_small(0u)};      // on no curve, and not the identity
    edp_store(raw, 1, 0, acc);
  } else {
    fe enc = ed_encode(acc);
    if (broken) {
#pragma unroll
      for (int j = 0; j < 8; ++j) enc.w[j] = 0xffffffffu;                // y >= p: no encoding
    }
    ed_store32(out, enc, out_aligned);
  }
  finite[0] = (uint8_t)((fin || broken) ? 1 : 0);
  if (invalid) invalid[0] = bad;
}

// ---- hashing.  SHA-512(R || A || M) as k_ed25519.hip has it, word for word (that unit keeps its own: its kernels' listings are pinned)
ECS_DEV size_t ed_lane_len(size_t i, size_t msg_bytes, size_t stride, const uint32_t* __restrict__ lens) {
  if (!lens) return msg_bytes;
  const size_t len = lens[i];
  return len < stride ? len : stride;
}
ECS_DEV void ed_be_words(const fe& x, uint64_t* be) {
#pragma unroll
  for (int j = 0; j < 4; ++j) be[j] = sha512_join(__builtin_bswap32(x.w[2 * j]), __builtin_bswap32(x.w[2 * j + 1]));
}
ECS_DEV fe ed_digest_half(const sha512_state& s, int half) {
  fe r;
#pragma unroll
  for (int j = 0; j < 4; ++j) { r.w[2 * j] = __builtin_bswap32((uint32_t)(s.h[4 * half + j] >> 32)); r.w[2 * j + 1] = __builtin_bswap32((uint32_t)s.h[4 * half + j]); }
  return r;
}
template <int PW> ECS_DEV sha512_state ed_hash(const uint64_t (&head)[PW], const uint8_t* __restrict__ p, size_t len, uint32_t aligned) {
  sha512_state s = sha512_iv();
  const size_t total = 8 * PW + len, blocks = (total + 17 + 127) / 128;
#pragma unroll 1
  for (size_t b = 0; b < blocks; ++b) {
    sha512_block m;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      uint64_t w = 0;
      const size_t pos = 128 * b + 8 * j;                      // of the word in the stream
      if (pos >= (size_t)(8 * PW)) {
        const size_t off = pos - 8 * PW;                       // ... and in the message: a multiple of 8
        if (off + 8 <= len) {                                  // a whole word of message
          if (aligned) {
            const uint32_t* q = reinterpret_cast<const uint32_t*>(p + off);
            w = sha512_join(__builtin_bswap32(q[0]), __builtin_bswap32(q[1]));
          } else {
#pragma unroll
            for (int t = 0; t < 8; ++t) w = (w << 8) | (uint64_t)p[off + t];
          }
        } else if (off <= len) {                               // the word the message ends in: up to 7 bytes and 0x80
#pragma unroll
          for (int t = 0; t < 8; ++t) {
            uint64_t byte = 0;
            if (off + t < len) byte = p[off + t];
            else if (off + t == len) byte = 0x80u;
            w = (w << 8) | byte;
          }
        }
      }
      if (j < PW) w = b == 0 ? head[j < PW ? j : 0] : w;       // the head's words, by position
      m.w[j] = w;
    }
    if (b + 1 == blocks) m.w[15] = (uint64_t)total * 8u;       // (the 0x80 and 16 length bytes fit by the choice of `blocks`: words 14 and 15 were zero)
    sha512_compress(s, m);
  }
  return s;
}
ECS_DEV sha512_state ed_challenge(const fe& R, const fe& A, const uint8_t* __restrict__ p, size_t len, uint32_t aligned) {
  uint64_t head[8];
  ed_be_words(R, head); ed_be_words(A, head + 4);
  return ed_hash<8>(head, p, len, aligned);
}
ECS_DEV uint32_t ed_bytes_equal_mask(const fe& a, const fe& b) {
  uint32_t d = 0;
#pragma unroll
  for (int q = 0; q < 8; ++q) d |= a.w[q] ^ b.w[q];
  return (uint32_t)((int32_t)((d | (0u - d)) ^ 0x80000000u) >> 31);
}
// all ones where enc is one of the eight encodings of the points of order 1, 2, 4 and 8 (k_ed25519.hip's list)
ECS_DEV uint32_t ed_small_order_mask(const fe& enc) {
  constexpr uint32_t S[3][8] = {
      {0xffffffecu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0x7fffffffu},      // y = p - 1: order 2
      {0x706a17c7u, 0x4fd84d3du, 0x760b3cbau, 0x0f67100du, 0xfa53202au, 0xc6cc392cu, 0x77fdc74eu, 0x7a03ac92u},      // order 8
      {0x8f95e826u, 0xb027b2c2u, 0x89f4c345u, 0xf098eff2u, 0x05acdfd5u, 0x3933c6d3u, 0x880238b1u, 0x05fc536du}};     // order 8
  fe y = enc;
  y.w[7] &= 0x7fffffffu;                                       // y = 0 and the two of order 8 are listed with either sign, 1 and p - 1 as they are (x = 0)
  uint32_t hit = ed_bytes_equal_mask(y, fe25519_small(0u)) | ed_bytes_equal_mask(enc, fe25519_small(1u));
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    fe c;
#pragma unroll
    for (int q = 0; q < 8; ++q) c.w[q] = S[k][q];
    hit |= ed_bytes_equal_mask(k == 0 ? enc : y, c);
  }
  return hit;
}

// The SHA-256 state after the block SHA256(tag) || SHA256(tag), tag = "ecsimd/ed25519-batch/leaf", ".../node", ".../seed", ".../a"
// (batch_tree.cuh's order)
struct ed25519_batch_consts {
  static constexpr uint32_t ED25519_BATCH_MID[4][8] = {
      {0xee16ee5du, 0xfd4513eeu, 0x03feb5f3u, 0xa8a1dbf5u, 0x42669db8u, 0x6bb7c4f7u, 0xf78e9b7fu, 0x4be5fc49u},
      {0xdfca4714u, 0xd1e432edu, 0xe53f521eu, 0xfd2c0f7du, 0xea07f9bcu, 0xdcdb2e3fu, 0xf58a9513u, 0x143b726bu},
      {0xcfc6f938u, 0x3799d0b8u, 0x5714f5acu, 0xda6cbc6cu, 0x3f88375au, 0x4fff5ebau, 0x8b89d0eau, 0xbf040506u},
      {0xbd9e8bddu, 0xb0ed2b25u, 0x33235b06u, 0xdcf30e0du, 0x5b34f636u, 0x98621840u, 0xe3843d0bu, 0x7c827d3cu}};
  ECS_DEV static uint32_t mid(int tag, int j) { return ED25519_BATCH_MID[tag][j]; }
};
using TAGS = ed25519_batch_consts;
// H_leaf(D || s): D's 64 bytes are one block; s (32 bytes as given, s.w[j] = bytes 4 j .. 4 j + 3) and the padding the second.  Digests are held as
// sha_digest_fe leaves them: the big-endian integer of the 32 bytes.
ECS_DEV fe hash_leaf(const sha512_state& D, const fe& s) {
  sha256_state st = mid<TAGS, BATCH_LEAF>();
  sha256_block m;
#pragma unroll
  for (int j = 0; j < 8; ++j) { m.w[2 * j] = (uint32_t)(D.h[j] >> 32); m.w[2 * j + 1] = (uint32_t)D.h[j]; }
  sha256_compress(st, m);
#pragma unroll
  for (int j = 0; j < 8; ++j) m.w[j] = __builtin_bswap32(s.w[j]);
  m.w[8] = 0x80000000u;
#pragma unroll
  for (int j = 9; j < 15; ++j) m.w[j] = 0u;
  m.w[15] = (64u + 96u) * 8u;
  sha256_compress(st, m);
  return sha_digest_fe(st);
}
// ---- the batch
__global__ void __launch_bounds__(BLOCK) k_edb_front(gmod M, const uint8_t* __restrict__ pk, uint32_t pk_aligned, const uint8_t* __restrict__ sig, uint32_t sig_aligned, MSG_ARGS,
                                                     uint32_t reject_small, uint64_t* __restrict__ hv, uint64_t* __restrict__ leafv, uint64_t* __restrict__ Aenc,
                                                     uint64_t* __restrict__ Renc, uint8_t* __restrict__ valid, uint32_t* __restrict__ malformed, size_t n) {
  GID;
  const fe A = ed_load32(pk + 32 * i, pk_aligned), R = ed_load32(sig + 64 * i, sig_aligned), s = ed_load32(sig + 64 * i + 32, sig_aligned);
  const sha512_state D = ed_challenge(R, A, msg + i * stride, ed_lane_len(i, msg_bytes, stride, lens), aligned);
  fe_store(hv, i, ed_sc_reduce512(ed_digest_half(D, 0), ed_digest_half(D, 1), M));
  fe_store(leafv, i, hash_leaf(D, s));
  fe_store(Aenc, i, A); fe_store(Renc, i, R);
  uint32_t ok = ed_sc_below_L(s);
  if (reject_small) ok &= ~(ed_small_order_mask(A) | ed_small_order_mask(R));
  if (!ok) atomicAdd(malformed, 1u);
  valid[i] = (uint8_t)(ok & 1u);
}
__global__ void __launch_bounds__(BLOCK) k_edb_node(const uint64_t* __restrict__ in, size_t count, uint64_t* __restrict__ out, size_t n) {
  GID;
  batch_node<TAGS>(in, count, out, i);
}
__global__ void __launch_bounds__(64) k_edb_seed(const uint64_t* __restrict__ root, uint64_t n, ed25519_batch_head* __restrict__ head) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  batch_seed<TAGS>(root, n, head->seed);
}
__global__ void __launch_bounds__(BLOCK) k_edb_scalars(gmod M, const ed25519_batch_head* __restrict__ head, const uint64_t* __restrict__ hv, const uint8_t* __restrict__ sig,
                                                       uint32_t sig_aligned, const uint8_t* __restrict__ valid, uint64_t* __restrict__ zv, uint64_t* __restrict__ zhv,
                                                       uint64_t* __restrict__ zsv, size_t n) {
  GID;
  const fe z = batch_randomizer<TAGS>(head->seed, i);
  fe h = fe_load(hv, i), s = ed_load32(sig + 64 * i + 32, sig_aligned);
  if (!valid[i]) { h = fe25519_small(0u); s = fe25519_small(0u); }    // (a malformed lane's s may be >= L: g_mul's operands stay below L)
  const fe zR = batch_randomizer_mgry(z, M);
  fe_store(zv, i, z);
  if (zhv) { fe_store(zhv, i, g_mul(zR, h, M)); fe_store(zsv, i, g_mul(zR, s, M)); }
}
// out[i] = the sum of in[16 i ..] modulo L.  benc != nullptr: the last level (one lane): out[0] = L - sum, 0 staying 0, and benc[0] = the encoding of B.
__global__ void __launch_bounds__(BLOCK) k_edb_sum(gmod M, const uint64_t* __restrict__ in, size_t count, uint64_t* __restrict__ out, uint64_t* __restrict__ benc, size_t n) {
  GID;
  const fe acc = batch_sum(M, in, count, i, benc != nullptr);
  if (benc) {
    fe b;
#pragma unroll
    for (int q = 0; q < 8; ++q) b.w[q] = 0x66666666u;
    b.w[0] = 0x66666658u;                                             // y = 4 / 5, x even
    fe_store(benc, 0, b);
  }
  fe_store(out, i, acc);
}
__global__ void __launch_bounds__(64) k_edb_accept(const ed25519_batch_head* __restrict__ head, uint8_t* __restrict__ okv) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const bool clean = head->malformed == 0u && head->invalid[0] == 0u && head->invalid[1] == 0u;
  ed_point p = ed_add(edp_load(head->sum[0], 1, 0), edp_load(head->sum[1], 1, 0));
  ed_dbl_nt(p); ed_dbl_nt(p); ed_dbl_nt(p);
  okv[0] = (uint8_t)((clean && ed_identity_mask(p)) ? 1 : 0);
}

// ---- the per-lane cofactored rule
__global__ void __launch_bounds__(BLOCK) k_edc_front(gmod M, const uint8_t* __restrict__ pk, uint32_t pk_aligned, const uint8_t* __restrict__ sig, uint32_t sig_aligned, MSG_ARGS,
                                                     uint32_t reject_small, uint64_t* __restrict__ sv, uint64_t* __restrict__ hv, uint64_t* __restrict__ rxy,
                                                     uint4* __restrict__ table, uint8_t* __restrict__ valid, size_t n) {
  GID;
  const fe A = ed_load32(pk + 32 * i, pk_aligned), R = ed_load32(sig + 64 * i, sig_aligned), s = ed_load32(sig + 64 * i + 32, sig_aligned);
  ed_point P, Q;
  uint32_t ok = ed_decode(P, A) & ed_sc_below_L(s);
  ok &= ed_decode(Q, R);
  if (reject_small) ok &= ~(ed_small_order_mask(A) | ed_small_order_mask(R));
  valid[i] = (uint8_t)(ok & 1u);
  if (!ok) return;                                             // (the loop kernel does not read a refused lane's scalars, point or table)
  fe_store(sv, i, s);
  const sha512_state D = ed_challenge(R, A, msg + i * stride, ed_lane_len(i, msg_bytes, stride, lens), aligned);
  fe_store(hv, i, ed_sc_reduce512(ed_digest_half(D, 0), ed_digest_half(D, 1), M));
  fe_store(rxy, i, Q.X); fe_store(rxy, n + i, Q.Y);
  ed_table_build(table, n, i, ed_neg(P));
}
__global__ void __launch_bounds__(BLOCK) k_edc_loop(const uint64_t* __restrict__ sv, const uint64_t* __restrict__ hv, const uint64_t* __restrict__ rxy,
                                                    const uint4* __restrict__ table, const uint8_t* __restrict__ valid, uint8_t* __restrict__ okv, size_t n) {
  GID;
  if (!valid[i]) { okv[i] = 0; return; }
  ed_point p = ed_straus_vartime(fe_load(sv, i), fe_load(hv, i), table, n, i);
  const fe x = fe_load(rxy, i), y = fe_load(rxy, n + i);
  const ed_point negR = {fe25519_neg(x), y, fe25519_small(1u), fe25519_neg(fe25519_mul(x, y))};
  p = ed_add(p, negR);
  ed_dbl_nt(p); ed_dbl_nt(p); ed_dbl_nt(p);
  okv[i] = (uint8_t)(ed_identity_mask(p) & 1u);
}
}  // namespace

namespace launch {
static_assert(sizeof(ed25519_batch_head) == 304 && sizeof(ed25519_batch_head) % 16 == 0, "ed25519_batch_head: zeroed 16 bytes per lane");
static uint32_t word_aligned(const void* p, size_t stride_bytes = 0) { return ((reinterpret_cast<uintptr_t>(p) | stride_bytes) & 3u) == 0 ? 1u : 0u; }
static dim3 grid_of(size_t lanes, size_t y = 1) { return dim3((unsigned)((lanes + BLOCK - 1) / BLOCK), (unsigned)y); }
static size_t fan_lanes(size_t count) { return (count + BATCH_FAN - 1) / BATCH_FAN; }

void ed25519_msm_launch::digits(hipStream_t s, const uint8_t* k, const uint8_t* pts, uint64_t* kk, uint64_t* pre, uint32_t* hist, uint32_t* counter, size_t n, int bits, int c, int windows) {
  hipLaunchKernelGGL(k_edm_digits, grid_of(n), dim3(BLOCK), 0, s, k, word_aligned(k), pts, word_aligned(pts), kk, pre, hist, counter, n, bits, c, windows);
}
void ed25519_msm_launch::slices(hipStream_t s, const uint32_t* sorted, const uint64_t* kk, const uint64_t* pre, const uint32_t* start, uint64_t* buckets, uint64_t* partial,
                                uint32_t* broken, size_t n, size_t T, size_t L, size_t slices, int c, size_t K) {
  hipLaunchKernelGGL(k_edm_slices, grid_of(slices), dim3(BLOCK), 0, s, sorted, kk, pre, start, buckets, partial, broken, n, T, L, slices, c, K);
}
void ed25519_msm_launch::combine(hipStream_t s, const uint32_t* start, uint64_t* buckets, const uint64_t* partial, uint32_t* broken, size_t L, size_t slices, int c, size_t K) {
  hipLaunchKernelGGL(k_edm_combine, grid_of(K), dim3(BLOCK), 0, s, start, buckets, partial, broken, L, slices, c, K);
}
void ed25519_msm_launch::chunks(hipStream_t s, const uint64_t* buckets, uint64_t* out, size_t lanes, size_t per_window, int c, int m, size_t K) {
  hipLaunchKernelGGL(k_edm_chunks, grid_of(lanes), dim3(BLOCK), 0, s, buckets, out, lanes, per_window, c, m, K);
}
void ed25519_msm_launch::tree(hipStream_t s, uint64_t* arr, size_t total, size_t count, size_t stride, size_t groups, size_t lanes, int fan) {
  hipLaunchKernelGGL(k_edm_tree, grid_of(lanes, groups), dim3(BLOCK), 0, s, arr, total, count, stride, lanes, fan);
}
void ed25519_msm_launch::finish(hipStream_t s, const uint64_t* arr, size_t total, size_t stride, int windows, int c, const uint32_t* counter, uint8_t* out, uint64_t* raw,
                                uint8_t* finite, uint32_t* invalid) {
  hipLaunchKernelGGL(k_edm_final, dim3(1), dim3(64), 0, s, arr, total, stride, windows, c, counter, out, word_aligned(out), raw, finite, invalid);
}
void ed25519_batch_front(hipStream_t s, const gmod& L, const uint8_t* pk, const uint8_t* sig, const uint8_t* msg, size_t msg_bytes, size_t stride_bytes, const uint32_t* lens,
                         bool reject_small_order, uint64_t* h, uint64_t* leaf, uint64_t* Aenc, uint64_t* Renc, uint8_t* valid, ed25519_batch_head* head, size_t n) {
  hipLaunchKernelGGL(k_edb_front, grid_of(n), dim3(BLOCK), 0, s, L, pk, word_aligned(pk), sig, word_aligned(sig), msg, msg_bytes, stride_bytes, lens, word_aligned(msg, stride_bytes),
                     reject_small_order ? 1u : 0u, h, leaf, Aenc, Renc, valid, &head->malformed, n);
}
void ed25519_batch_node(hipStream_t s, const uint64_t* in, size_t count, uint64_t* out) {
  hipLaunchKernelGGL(k_edb_node, grid_of(fan_lanes(count)), dim3(BLOCK), 0, s, in, count, out, fan_lanes(count));
}
void ed25519_batch_seed(hipStream_t s, const uint64_t* root, size_t n, ed25519_batch_head* head) {
  hipLaunchKernelGGL(k_edb_seed, dim3(1), dim3(64), 0, s, root, (uint64_t)n, head);
}
void ed25519_batch_scalars(hipStream_t s, const gmod& L, const ed25519_batch_head* head, const uint64_t* h, const uint8_t* sig, const uint8_t* valid, uint64_t* z, uint64_t* zh,
                           uint64_t* zs, size_t n) {
  hipLaunchKernelGGL(k_edb_scalars, grid_of(n), dim3(BLOCK), 0, s, L, head, h, sig, word_aligned(sig), valid, z, zh, zs, n);
}
void ed25519_batch_sum(hipStream_t s, const gmod& L, const uint64_t* in, size_t count, uint64_t* out, uint64_t* benc) {
  hipLaunchKernelGGL(k_edb_sum, grid_of(fan_lanes(count)), dim3(BLOCK), 0, s, L, in, count, out, benc, fan_lanes(count));
}
void ed25519_batch_accept(hipStream_t s, const ed25519_batch_head* head, uint8_t* ok) {
  hipLaunchKernelGGL(k_edb_accept, dim3(1), dim3(64), 0, s, head, ok);
}
void ed25519_cofactored_front(hipStream_t s, const gmod& L, const uint8_t* pk, const uint8_t* sig, const uint8_t* msg, size_t msg_bytes, size_t stride_bytes, const uint32_t* lens,
                              bool reject_small_order, uint64_t* sv, uint64_t* hv, uint64_t* rxy, void* table, uint8_t* valid, size_t n) {
  hipLaunchKernelGGL(k_edc_front, grid_of(n), dim3(BLOCK), 0, s, L, pk, word_aligned(pk), sig, word_aligned(sig), msg, msg_bytes, stride_bytes, lens, word_aligned(msg, stride_bytes),
                     reject_small_order ? 1u : 0u, sv, hv, rxy, static_cast<uint4*>(table), valid, n);
}
void ed25519_cofactored_loop(hipStream_t s, const uint64_t* sv, const uint64_t* hv, const uint64_t* rxy, const void* table, const uint8_t* valid, uint8_t* ok, size_t n) {
  hipLaunchKernelGGL(k_edc_loop, grid_of(n), dim3(BLOCK), 0, s, sv, hv, rxy, static_cast<const uint4*>(table), valid, ok, n);
}
}  // namespace launch
}  // namespace ecsimd_hip
