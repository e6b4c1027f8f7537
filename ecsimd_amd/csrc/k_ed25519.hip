// k_ed25519.hip -- Ed25519 (RFC 8032, pure): the kernels behind ecsimd_ed25519_pubkey / _sign / _verify / _raw.  fe25519.cuh is the field, ed25519.cuh the
// group, its two scalar-multiplication loops and the scalars modulo L; sha512.cuh the compression.
//
// Hashing: SHA-512 over a short fixed head held in registers (the 32-byte seed; the 32-byte prefix; R || A, 64 bytes) with the message absorbed behind it,
// one block loop for any length -- the head's words are placed by compile-time position, the message's 64-bit words are whole-word loads while they lie
// inside the lane's message (no byte at or behind its end is loaded) and byte loads for the word it ends in.  Lengths may differ per lane (lens); lengths,
// strides and alignment are PUBLIC, and they alone decide the block loop's trip count and every load's address and lane mask.
//
// Signing and key derivation, SECRET data (the seed, h, a, the prefix, r, both hash states, the products and their inverses): selects by masks only, no
// branch, address or lane mask made of them, nothing declassified (tools/ct_check.py check_secret_flow holds the ISA to that), no scratch memory.
//   * k_ed_secret_front<SIGN>  h = SHA-512(seed); a = the clamped low half, stored reduced modulo L (B has order L, and s = r + k a is modulo L); with SIGN
//                              also r = SHA-512(prefix || M) mod L, the prefix never leaving its registers.
//   * k_ed_base_ct             the encoding of [k]B for each of m scalars (the comb of ed25519.cuh, one inversion): a then r for signing, 2 m lanes.
//   * k_ed_sign_finish         k = SHA-512(R || A || M) mod L, s = r + k a mod L; writes R || s and, where asked, A.
// Verification, PUBLIC data:
//   * k_ed_verify_front        valid = s < L && A decodes (&& neither A nor R is a small-order encoding, with the flag); h = SHA-512(R || A || M) mod L;
//                              the lane's table of 1 .. 8 times -A.
//   * k_ed_verify_loop         ok = valid && encode([s]B + [h](-A)) == the bytes of R.  R is never decompressed.
//   * k_ed_raw                 one function of the layers below on raw operands (ecsimd_ed25519_raw).
#include "kernels.h"
#include "sha512.cuh"
#include "ed25519.cuh"

namespace ecsimd_hip {
namespace {
using launch::BLOCK;
#define GID size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x; if (i >= n) return
// The messages as the kernels see them: lane i's bytes at msg + i * stride, lens[i] of them (never more than stride) where lens is given, else msg_bytes;
// aligned: msg and stride are multiples of 4.
#define MSG_ARGS const uint8_t* __restrict__ msg, size_t msg_bytes, size_t stride, const uint32_t* __restrict__ lens, uint32_t aligned
#define MSG_PASS msg, msg_bytes, stride, lens, aligned
ECS_DEV size_t ed_lane_len(size_t i, size_t msg_bytes, size_t stride, const uint32_t* __restrict__ lens) {
  if (!lens) return msg_bytes;
  const size_t len = lens[i];
  return len < stride ? len : stride;
}

// 32 little-endian bytes held as an fe <-> the four big-endian 64-bit words SHA-512 reads them as
ECS_DEV void ed_be_words(const fe& x, uint64_t* be) {
#pragma unroll
  for (int j = 0; j < 4; ++j) be[j] = sha512_join(__builtin_bswap32(x.w[2 * j]), __builtin_bswap32(x.w[2 * j + 1]));
}
// digest bytes 32 half .. 32 half + 31 as a little-endian integer
ECS_DEV fe ed_digest_half(const sha512_state& s, int half) {
  fe r;
#pragma unroll
  for (int j = 0; j < 4; ++j) { r.w[2 * j] = __builtin_bswap32((uint32_t)(s.h[4 * half + j] >> 32)); r.w[2 * j + 1] = __builtin_bswap32((uint32_t)s.h[4 * half + j]); }
  return r;
}
// SHA-512(head || message): head = PW 64-bit words in registers, the message len bytes at p
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
// SHA-512(x || y || message) mod L, x and y 32 bytes each in registers
ECS_DEV fe ed_hash_2x32_mod_L(const fe& x, const fe& y, const uint8_t* __restrict__ p, size_t len, uint32_t aligned, const gmod& M) {
  uint64_t head[8];
  ed_be_words(x, head); ed_be_words(y, head + 4);
  const sha512_state s = ed_hash<8>(head, p, len, aligned);
  return ed_sc_reduce512(ed_digest_half(s, 0), ed_digest_half(s, 1), M);
}
ECS_DEV uint32_t ed_bytes_equal_mask(const fe& a, const fe& b) {
  uint32_t d = 0;
#pragma unroll
  for (int q = 0; q < 8; ++q) d |= a.w[q] ^ b.w[q];
  return (uint32_t)((int32_t)((d | (0u - d)) ^ 0x80000000u) >> 31);
}
// all ones where enc is one of the eight encodings of the points of order 1, 2, 4 and 8
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

// ---- key derivation and signing (secret data)
template <bool SIGN>
__global__ void __launch_bounds__(BLOCK) k_ed_secret_front(gmod M, const uint8_t* __restrict__ seed, uint32_t seed_aligned, MSG_ARGS, uint64_t* __restrict__ av,
                                                           uint64_t* __restrict__ rv, size_t n) {
  GID;
  uint64_t head[4];
  ed_be_words(ed_load32(seed + 32 * i, seed_aligned), head);
  const sha512_state h = ed_hash<4>(head, nullptr, 0, 0u);
  fe a = ed_digest_half(h, 0);
  a.w[0] &= 0xfffffff8u;
  a.w[7] = (a.w[7] & 0x7fffffffu) | 0x40000000u;
  fe_store(av, i, ed_sc_reduce256(a, M));
  if constexpr (SIGN) {
    const uint64_t prefix[4] = {h.h[4], h.h[5], h.h[6], h.h[7]};
    const sha512_state t = ed_hash<4>(prefix, msg + i * stride, ed_lane_len(i, msg_bytes, stride, lens), aligned);
    fe_store(rv, i, ed_sc_reduce512(ed_digest_half(t, 0), ed_digest_half(t, 1), M));
  }
}
__global__ void __launch_bounds__(BLOCK) k_ed_base_ct(const uint64_t* __restrict__ kv, uint8_t* __restrict__ out, uint32_t out_aligned, size_t n) {
  GID;
  ed_store32(out + 32 * i, ed_encode(ed_base_ct(fe_load(kv, i))), out_aligned);
}
// encA / encR: the encodings k_ed_base_ct left in the workspace (word aligned)
__global__ void __launch_bounds__(BLOCK) k_ed_sign_finish(gmod M, const uint64_t* __restrict__ av, const uint64_t* __restrict__ rv, const uint8_t* __restrict__ encA,
                                                          const uint8_t* __restrict__ encR, MSG_ARGS, uint8_t* __restrict__ sig, uint32_t sig_aligned,
                                                          uint8_t* __restrict__ pk, uint32_t pk_aligned, size_t n) {
  GID;
  const fe A = ed_load32(encA + 32 * i, 1u), R = ed_load32(encR + 32 * i, 1u);
  const fe k = ed_hash_2x32_mod_L(R, A, msg + i * stride, ed_lane_len(i, msg_bytes, stride, lens), aligned, M);
  const fe s = ed_sc_muladd(fe_load(rv, i), k, fe_load(av, i), M);
  ed_store32(sig + 64 * i, R, sig_aligned);
  ed_store32(sig + 64 * i + 32, s, sig_aligned);
  if (pk) ed_store32(pk + 32 * i, A, pk_aligned);
}

// ---- verification (public data)
__global__ void __launch_bounds__(BLOCK) k_ed_verify_front(gmod M, const uint8_t* __restrict__ pk, uint32_t pk_aligned, const uint8_t* __restrict__ sig, uint32_t sig_aligned,
                                                           MSG_ARGS, uint32_t reject_small, uint64_t* __restrict__ sv, uint64_t* __restrict__ hv, uint4* __restrict__ table,
                                                           uint8_t* __restrict__ valid, size_t n) {
  GID;
  const fe A = ed_load32(pk + 32 * i, pk_aligned), R = ed_load32(sig + 64 * i, sig_aligned), s = ed_load32(sig + 64 * i + 32, sig_aligned);
  ed_point P;
  uint32_t ok = ed_decode(P, A) & ed_sc_below_L(s);
  if (reject_small) ok &= ~(ed_small_order_mask(A) | ed_small_order_mask(R));
  valid[i] = (uint8_t)(ok & 1u);
  if (!ok) return;                                             // (the loop kernel does not read a refused lane's scalars or table)
  fe_store(sv, i, s);
  fe_store(hv, i, ed_hash_2x32_mod_L(R, A, msg + i * stride, ed_lane_len(i, msg_bytes, stride, lens), aligned, M));
  ed_table_build(table, n, i, ed_neg(P));
}
__global__ void __launch_bounds__(BLOCK) k_ed_verify_loop(const uint64_t* __restrict__ sv, const uint64_t* __restrict__ hv, const uint4* __restrict__ table,
                                                          const uint8_t* __restrict__ valid, const uint8_t* __restrict__ sig, uint32_t sig_aligned,
                                                          uint8_t* __restrict__ okv, size_t n) {
  GID;
  if (!valid[i]) { okv[i] = 0; return; }
  const fe enc = ed_encode(ed_straus_vartime(fe_load(sv, i), fe_load(hv, i), table, n, i));
  okv[i] = (uint8_t)(ed_bytes_equal_mask(enc, ed_load32(sig + 64 * i, sig_aligned)) & 1u);
}

// ---- one function per layer on raw operands: records of 32-byte little-endian values, launch::ed_raw_inputs(op) of them in and ed_raw_outputs(op) out per lane
ECS_DEV fe ed_flag_record(uint32_t mask) { return fe25519_small(mask & 1u); }
__global__ void __launch_bounds__(BLOCK) k_ed_raw(gmod M, int op, const uint8_t* __restrict__ in, uint8_t* __restrict__ out, uint32_t aligned, uint4* __restrict__ table, size_t n) {
  GID;
  const int ni = launch::ed_raw_inputs(op), no = launch::ed_raw_outputs(op);
  const uint8_t* ip = in + (size_t)32 * ni * i;
  uint8_t* op_ = out + (size_t)32 * no * i;
  const fe a = ed_load32(ip, aligned);
  const fe b = ni > 1 ? ed_load32(ip + 32, aligned) : fe25519_small(0u);
  fe r = fe25519_small(0u), flag = fe25519_small(0u);
  switch (op) {
    case launch::ED_RAW_FE_MUL: r = fe25519_canon(fe25519_mul(a, b)); break;
    case launch::ED_RAW_FE_SQR: r = fe25519_canon(fe25519_sqr(a)); break;
    case launch::ED_RAW_FE_ADD: r = fe25519_canon(fe25519_add(a, b)); break;
    case launch::ED_RAW_FE_SUB: r = fe25519_canon(fe25519_sub(a, b)); break;
    case launch::ED_RAW_FE_NEG: r = fe25519_canon(fe25519_neg(a)); break;
    case launch::ED_RAW_FE_INVERT: r = fe25519_canon(fe25519_invert(a)); break;
    case launch::ED_RAW_FE_CANON: r = fe25519_canon(a); break;
    case launch::ED_RAW_SQRT_RATIO: { fe x; flag = ed_flag_record(fe25519_sqrt_ratio(x, a, b)); r = fe25519_canon(x); break; }
    case launch::ED_RAW_DECODE_ENCODE: { ed_point p; const uint32_t ok = ed_decode(p, a); flag = ed_flag_record(ok); r = fe25519_select(ok, ed_encode(p), r); break; }
    case launch::ED_RAW_POINT_ADD: {
      ed_point p, q; const uint32_t ok = ed_decode(p, a) & ed_decode(q, b);
      flag = ed_flag_record(ok); r = fe25519_select(ok, ed_encode(ed_add(p, q)), r); break; }
    case launch::ED_RAW_POINT_DBL: { ed_point p; const uint32_t ok = ed_decode(p, a); flag = ed_flag_record(ok); r = fe25519_select(ok, ed_encode(ed_dbl(p)), r); break; }
    case launch::ED_RAW_SC_REDUCE: r = ed_sc_reduce512(a, b, M); break;
    case launch::ED_RAW_BASE_MULT: r = ed_encode(ed_base_ct(ed_sc_reduce256(a, M))); break;
    case launch::ED_RAW_DOUBLE_MULT: {
      ed_point p; const uint32_t ok = ed_decode(p, ed_load32(ip + 64, aligned));
      flag = ed_flag_record(ok);
      if (ok) { ed_table_build(table, n, i, p); r = ed_encode(ed_straus_vartime(ed_sc_reduce256(a, M), ed_sc_reduce256(b, M), table, n, i)); }
      break; }
    default: break;
  }
  ed_store32(op_, r, aligned);
  if (no > 1) ed_store32(op_ + 32, flag, aligned);
}
}  // namespace

namespace launch {
static uint32_t word_aligned(const void* p, size_t stride_bytes = 0) { return ((reinterpret_cast<uintptr_t>(p) | stride_bytes) & 3u) == 0 ? 1u : 0u; }
void ed25519_secret_front(hipStream_t s, const gmod& L, const uint8_t* seed, const uint8_t* msg, size_t msg_bytes, size_t stride_bytes, const uint32_t* lens, bool sign,
                          uint64_t* a, uint64_t* r, size_t n) {
  if (sign) hipLaunchKernelGGL(k_ed_secret_front<true>, grid_for(n), dim3(BLOCK), 0, s, L, seed, word_aligned(seed), msg, msg_bytes, stride_bytes, lens, word_aligned(msg, stride_bytes), a, r, n);
  else hipLaunchKernelGGL(k_ed_secret_front<false>, grid_for(n), dim3(BLOCK), 0, s, L, seed, word_aligned(seed), nullptr, (size_t)0, (size_t)0, nullptr, 0u, a, nullptr, n);
}
void ed25519_base_ct(hipStream_t s, const uint64_t* k, uint8_t* out32, size_t n) {
  hipLaunchKernelGGL(k_ed_base_ct, grid_for(n), dim3(BLOCK), 0, s, k, out32, word_aligned(out32), n);
}
void ed25519_sign_finish(hipStream_t s, const gmod& L, const uint64_t* a, const uint64_t* r, const uint8_t* encA, const uint8_t* encR, const uint8_t* msg, size_t msg_bytes,
                         size_t stride_bytes, const uint32_t* lens, uint8_t* sig, uint8_t* pk, size_t n) {
  hipLaunchKernelGGL(k_ed_sign_finish, grid_for(n), dim3(BLOCK), 0, s, L, a, r, encA, encR, msg, msg_bytes, stride_bytes, lens, word_aligned(msg, stride_bytes), sig, word_aligned(sig),
                     pk, word_aligned(pk), n);
}
void ed25519_verify_front(hipStream_t s, const gmod& L, const uint8_t* pk, const uint8_t* sig, const uint8_t* msg, size_t msg_bytes, size_t stride_bytes, const uint32_t* lens,
                          bool reject_small_order, uint64_t* sv, uint64_t* hv, void* table, uint8_t* valid, size_t n) {
  hipLaunchKernelGGL(k_ed_verify_front, grid_for(n), dim3(BLOCK), 0, s, L, pk, word_aligned(pk), sig, word_aligned(sig), msg, msg_bytes, stride_bytes, lens,
                     word_aligned(msg, stride_bytes), reject_small_order ? 1u : 0u, sv, hv, static_cast<uint4*>(table), valid, n);
}
void ed25519_verify_loop(hipStream_t s, const uint64_t* sv, const uint64_t* hv, const void* table, const uint8_t* valid, const uint8_t* sig, uint8_t* ok, size_t n) {
  hipLaunchKernelGGL(k_ed_verify_loop, grid_for(n), dim3(BLOCK), 0, s, sv, hv, static_cast<const uint4*>(table), valid, sig, word_aligned(sig), ok, n);
}
void ed25519_raw(hipStream_t s, const gmod& L, int op, const uint8_t* in, uint8_t* out, void* table, size_t n) {
  hipLaunchKernelGGL(k_ed_raw, grid_for(n), dim3(BLOCK), 0, s, L, op, in, out, word_aligned(in) & word_aligned(out), static_cast<uint4*>(table), n);
}
}  // namespace launch
}  // namespace ecsimd_hip
