// k_pbkdf2.hip -- PBKDF2 (RFC 8018 section 5.2) with HMAC-SHA-512 as the PRF, one (password, salt) pair per lane and one 64-byte output block per value of
// blockIdx.y: what BIP-39 makes a seed of (password = the sentence, salt = "mnemonic" || passphrase, c = 2048, dkLen = 64).
//
//   * k_pbkdf2<FIRST, LAST>   ONE kernel for the whole derivation and for its slices.
//       FIRST   the set-up: the password's key block (zero-padded up to 128 bytes, its SHA-512 beyond), the two midstates (hmac512_key_from), and
//               U_1 = HMAC(P, pre || salt || INT32BE(block)): the stream is absorbed behind the inner midstate block by block, the four counter bytes, the padding
//               bit and the bit length are placed in registers wherever the salt ends (the counter may straddle a block, the padding may open a block of its own).
//               T = U_1.  pre: eight bytes in front of the salt that no memory holds (BIP-39's "mnemonic"), or none.
//       !FIRST  the lane's inner midstate, outer midstate, U and T (256 B) come from the workspace.
//       the loop, `loops` times: U = HMAC(P, U) as ONE compression of sha512_tail_block64(U, 192) from the inner midstate and ONE of the same tail from the
//               outer midstate, T ^= U.  No load, no store, no LDS; the tail blocks are half constants, which the compiler folds into the unrolled rounds.  The
//               loop stays a loop (DESIGN.md section 4d has the listing's figures and those of the form that lost).
//       LAST    T's bytes, as many as dk_bytes leaves to this block, go to out + i * out_stride + 64 block.
//       !LAST   the four states go back to the workspace.
//
// PUBLIC: the lengths (pw_bytes / pw_lens, salt_bytes / salt_lens), loops, dk_bytes, strides, alignment.  They steer loads and the block loops, per lane where
// lens is given.  SECRET: the password's and the salt's bytes, the midstates, U, T, the workspace and the output: no branch, address or lane mask in force at a
// memory access is made of them and no bit is declassified (tools/ct_check.py check_secret_flow on the shipped ISA: tests/test_bip39_cpu.py).
#include "kernels.h"
#include "sha512.cuh"

namespace ecsimd_hip {
namespace {
using launch::BLOCK;

// bytes q0 .. q0 + 7 of the len bytes at p as a big-endian word, zeros behind the end (nothing behind it is read).  aligned: p and q0 are multiples of 4.
ECS_DEV uint64_t load_be64(const uint8_t* __restrict__ p, uint32_t len, uint32_t q0, bool aligned) {
  uint64_t w = 0;
  if (q0 + 8u <= len) {
    if (aligned) {
      const uint32_t* q = reinterpret_cast<const uint32_t*>(p + q0);
      w = sha512_join(__builtin_bswap32(q[0]), __builtin_bswap32(q[1]));
    } else {
#pragma unroll
      for (uint32_t t = 0; t < 8; ++t) w = (w << 8) | (uint64_t)p[q0 + t];
    }
  } else if (q0 < len) {
#pragma unroll
    for (uint32_t t = 0; t < 8; ++t) {
      uint64_t byte = 0;
      if (q0 + t < len) byte = p[q0 + t];
      w = (w << 8) | byte;
    }
  }
  return w;
}

// Block b of the stream  pre (pre_bytes: 0 or 8) || the len bytes at p || tail || zeros: tail holds at most five bytes at its top (the counter and 0x80, or
// 0x80 alone) and lands wherever the bytes end.  last: the stream's bit length goes into the block's last word (the caller's block count leaves it free).
ECS_DEV sha512_block stream_block(const uint8_t* __restrict__ p, uint32_t len, bool aligned, uint64_t pre, uint32_t pre_bytes, uint64_t tail, uint32_t b, bool last, uint64_t bits) {
  sha512_block m;
  const uint32_t end = pre_bytes + len;
#pragma unroll
  for (uint32_t j = 0; j < 16; ++j) {
    const uint32_t q0 = 128u * b + 8u * j;
    uint64_t w = q0 < pre_bytes ? pre : load_be64(p, len, q0 - pre_bytes, aligned);
    const int32_t d = (int32_t)(end - q0);                                          // where the tail starts, seen from this word
    if (d >= 0 && d < 8) w |= tail >> (8 * d);
    else if (d < 0 && d > -8) w |= tail << (8 * -d);
    m.w[j] = w;
  }
  if (last) m.w[15] = bits;
  return m;
}

// the four states of a (lane, block) unit in the workspace: sixteen 16-byte words, word j of unit u at ws[j * units + u]
struct pbkdf2_state { sha512_state inner, outer, u, t; };
ECS_DEV void state_store(uint4* __restrict__ ws, size_t units, size_t u, int k, const sha512_state& s) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const uint64_t a = s.h[2 * j], b = s.h[2 * j + 1];
    ws[(size_t)(4 * k + j) * units + u] = make_uint4((uint32_t)a, (uint32_t)(a >> 32), (uint32_t)b, (uint32_t)(b >> 32));
  }
}
ECS_DEV sha512_state state_load(const uint4* __restrict__ ws, size_t units, size_t u, int k) {
  sha512_state s;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const uint4 v = ws[(size_t)(4 * k + j) * units + u];
    s.h[2 * j] = sha512_join(v.y, v.x);
    s.h[2 * j + 1] = sha512_join(v.w, v.z);
  }
  return s;
}

enum { PW_ALIGNED = 1, SALT_ALIGNED = 2, OUT_ALIGNED = 4 };

// Lane i of the grid's x, output block block_first + blockIdx.y (counted from 0; RFC 8018 counts from 1); units = n * gridDim.y.
template <bool FIRST, bool LAST>
__global__ void __launch_bounds__(BLOCK) k_pbkdf2(const uint8_t* __restrict__ pw, uint32_t pw_bytes, size_t pw_stride, const uint32_t* __restrict__ pw_lens,
                                                  const uint8_t* __restrict__ salt, uint32_t salt_bytes, size_t salt_stride, const uint32_t* __restrict__ salt_lens,
                                                  uint64_t pre, uint32_t pre_bytes, uint32_t aligned, uint32_t block_first, uint32_t loops, uint4* __restrict__ ws, size_t units,
                                                  uint8_t* __restrict__ out, uint32_t dk_bytes, size_t out_stride, size_t n) {
  const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n) return;
  const size_t unit = (size_t)blockIdx.y * n + i;
  const uint32_t block = block_first + blockIdx.y;
  pbkdf2_state S;
  if constexpr (FIRST) {
    // the key block of the password
    uint32_t plen = pw_bytes;
    if (pw_lens) { plen = pw_lens[i]; plen = plen < pw_stride ? plen : (uint32_t)pw_stride; }             // never past the lane's own stride
    const uint8_t* pp = pw + i * pw_stride;
    const bool pa = (aligned & PW_ALIGNED) != 0;
    sha512_block kb;
    if (plen > 128u) {
      sha512_state ks = sha512_iv();
      const uint32_t blocks = (plen + 17u + 127u) / 128u;
#pragma unroll 1
      for (uint32_t b = 0; b < blocks; ++b) sha512_compress(ks, stream_block(pp, plen, pa, 0u, 0u, 0x80ull << 56, b, b + 1u == blocks, (uint64_t)plen * 8u));
#pragma unroll
      for (int j = 0; j < 8; ++j) { kb.w[j] = ks.h[j]; kb.w[8 + j] = 0u; }
    } else {
#pragma unroll
      for (uint32_t j = 0; j < 16; ++j) kb.w[j] = load_be64(pp, plen, 8u * j, pa);
    }
    const hmac512_key K = hmac512_key_from(kb);
    S.inner = K.inner; S.outer = K.outer;
    // U_1: pre || salt || INT32BE(block + 1) behind the ipad block
    uint32_t slen = salt_bytes;
    if (salt_lens) { slen = salt_lens[i]; slen = slen < salt_stride ? slen : (uint32_t)salt_stride; }
    const uint8_t* sp = salt + i * salt_stride;                                                             // salt_stride == 0: one salt for the call
    const uint32_t end = pre_bytes + slen;
    const uint32_t blocks = (end + 4u + 17u + 127u) / 128u;
    const uint64_t tail = ((uint64_t)(block + 1u) << 32) | (0x80ull << 24);
    sha512_state in = S.inner;
#pragma unroll 1
    for (uint32_t b = 0; b < blocks; ++b)
      sha512_compress(in, stream_block(sp, slen, (aligned & SALT_ALIGNED) != 0, pre, pre_bytes, tail, b, b + 1u == blocks, (128ull + end + 4u) * 8u));
    S.u = hmac512_finish(S.outer, in);
    S.t = S.u;
  } else {
    S.inner = state_load(ws, units, unit, 0); S.outer = state_load(ws, units, unit, 1); S.u = state_load(ws, units, unit, 2); S.t = state_load(ws, units, unit, 3);
  }
#pragma unroll 1
  for (uint32_t r = 0; r < loops; ++r) {
    sha512_state a = S.inner;
    sha512_compress(a, sha512_tail_block64(S.u, 192u));
    S.u = S.outer;
    sha512_compress(S.u, sha512_tail_block64(a, 192u));
#pragma unroll
    for (int j = 0; j < 8; ++j) S.t.h[j] ^= S.u.h[j];
  }
  if constexpr (LAST) {
    const uint32_t take = dk_bytes - 64u * block < 64u ? dk_bytes - 64u * block : 64u;                      // the host launches no block at or behind dk_bytes
    uint8_t* o = out + i * out_stride + 64u * (size_t)block;
#pragma unroll
    for (uint32_t j = 0; j < 8; ++j) {
      const uint64_t w = S.t.h[j];
      if ((aligned & OUT_ALIGNED) != 0 && 8u * j + 8u <= take) {
        uint32_t* q = reinterpret_cast<uint32_t*>(o + 8u * j);
        q[0] = __builtin_bswap32((uint32_t)(w >> 32)); q[1] = __builtin_bswap32((uint32_t)w);
      } else {
#pragma unroll
        for (uint32_t t = 0; t < 8; ++t)
          if (8u * j + t < take) o[8u * j + t] = (uint8_t)(w >> (56u - 8u * t));
      }
    }
  } else {
    state_store(ws, units, unit, 0, S.inner); state_store(ws, units, unit, 1, S.outer); state_store(ws, units, unit, 2, S.u); state_store(ws, units, unit, 3, S.t);
  }
}
}  // namespace

namespace launch {
static bool word_aligned(const void* p, size_t stride_bytes) { return ((reinterpret_cast<uintptr_t>(p) | stride_bytes) & 3u) == 0; }
void pbkdf2_hmac_sha512(hipStream_t s, bool first, bool last, const uint8_t* pw, size_t pw_bytes, size_t pw_stride_bytes, const uint32_t* pw_lens, const uint8_t* salt,
                        size_t salt_bytes, size_t salt_stride_bytes, const uint32_t* salt_lens, uint64_t pre, unsigned pre_bytes, unsigned block_first, unsigned blocks,
                        unsigned loops, void* state, uint8_t* out, size_t dk_bytes, size_t out_stride_bytes, size_t n) {
  const uint32_t aligned = (word_aligned(pw, pw_stride_bytes) ? PW_ALIGNED : 0) | (word_aligned(salt, salt_stride_bytes) ? SALT_ALIGNED : 0) |
                           (word_aligned(out, out_stride_bytes) ? OUT_ALIGNED : 0);
  const dim3 grid((unsigned)((n + BLOCK - 1) / BLOCK), blocks);
#define PBKDF2(F, L) hipLaunchKernelGGL((k_pbkdf2<F, L>), grid, dim3(BLOCK), 0, s, pw, (uint32_t)pw_bytes, pw_stride_bytes, pw_lens, salt, (uint32_t)salt_bytes, salt_stride_bytes, \
                                        salt_lens, pre, (uint32_t)pre_bytes, aligned, (uint32_t)block_first, (uint32_t)loops, static_cast<uint4*>(state), n * blocks, out,           \
                                        (uint32_t)dk_bytes, out_stride_bytes, n)
  if (first && last) PBKDF2(true, true); else if (first) PBKDF2(true, false); else if (last) PBKDF2(false, true); else PBKDF2(false, false);
#undef PBKDF2
}
}  // namespace launch
}  // namespace ecsimd_hip
