// k_sha256.hip -- SHA-256 over a batch of equal-length messages, and the RFC 6979 nonce generator (section 3.2, H = SHA-256, qlen = hlen = 256) on it.
//
//   * k_sha256          one message per lane, public data: blocks are read where the lane's message lies, the last one or two are padded in registers.
//   * k_rfc6979_first   steps a-g and the first candidate of step h: 16 compressions per lane -- the two midstates of the all-zero initial key are
//                       compile-time constants, every later key is compressed once into its ipad / opad midstates (hmac_key) and reused.
//   * k_rfc6979_retry   step h.3 for the lanes whose candidate was outside [1, n - 1]: K = HMAC_K(V || 00), V = HMAC_K(V), the next candidate
//                       T = HMAC_K(V): 8 compressions per further candidate, at most `cap` candidates per lane in all.
//
// Secrets: d, the HMAC state (K as its two midstates, V), every candidate and the nonce.  They stay out of every branch condition, address and lane mask
// in force at a memory access (tools/ct_check.py check_secret_flow on the shipped ISA) with ONE exception, the one RFC 6979 itself makes: its loop branches
// on "this candidate was in range".  That bit leaves the secret side through one named byte array, `retry`: k_rfc6979_first writes it, k_rfc6979_retry
// reads it back as public data, leaves where it is 0 and loops while it is 1.  A rejected candidate says nothing about the accepted one.
// Range checks are borrows turned into masks, results are selected by masks; ok = 0 and k = 0 where d is outside [1, n - 1] or the cap is exhausted.
#include "kernels.h"
#include "sha256.cuh"
#include "gfield.cuh"

namespace ecsimd_hip {
namespace {
using launch::BLOCK;
using launch::words8;
#define GID size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x; if (i >= n) return
// the retry byte as the loop sees it: device memory, re-read at every use (the address space is spelled out: a volatile access through a generic pointer is a flat one)
typedef __attribute__((address_space(1))) volatile uint8_t retry_byte;

// msg_bytes, stride and `aligned` (the base and the stride are multiples of 4) are the same for every lane: all the branches below are uniform.
__global__ void __launch_bounds__(BLOCK) k_sha256(const uint8_t* __restrict__ msg, size_t msg_bytes, size_t stride, uint64_t* __restrict__ out, size_t n, uint32_t aligned) {
  GID;
  sha256_state s = sha256_iv();
  sha256_absorb_message(s, msg + i * stride, msg_bytes, aligned, 0);
  fe_store(out, i, sha_digest_fe(s));
}

ECS_DEV fe words8_fe(const words8& a) {
  fe r;
#pragma unroll
  for (int k = 0; k < 8; ++k) r.w[k] = a.w[k];
  return r;
}
// all ones where 1 <= v < n
ECS_DEV uint32_t in_range_mask(const fe& v, const fe& N) {
  fe t;
  return sub8_3(t, v, N) & ~g_zero_mask(v);
}
ECS_DEV void state_store(uint4* __restrict__ st, size_t i, const hmac_key& K, const sha256_state& V) {
  uint4* p = st + 6 * i;
  p[0] = make_uint4(K.inner.h[0], K.inner.h[1], K.inner.h[2], K.inner.h[3]); p[1] = make_uint4(K.inner.h[4], K.inner.h[5], K.inner.h[6], K.inner.h[7]);
  p[2] = make_uint4(K.outer.h[0], K.outer.h[1], K.outer.h[2], K.outer.h[3]); p[3] = make_uint4(K.outer.h[4], K.outer.h[5], K.outer.h[6], K.outer.h[7]);
  p[4] = make_uint4(V.h[0], V.h[1], V.h[2], V.h[3]);                         p[5] = make_uint4(V.h[4], V.h[5], V.h[6], V.h[7]);
}
ECS_DEV void state_load(const uint4* __restrict__ st, size_t i, hmac_key& K, sha256_state& V) {
  const uint4* p = st + 6 * i;
  const uint4 a = p[0], b = p[1], c = p[2], d = p[3], e = p[4], f = p[5];
  K.inner.h[0] = a.x; K.inner.h[1] = a.y; K.inner.h[2] = a.z; K.inner.h[3] = a.w; K.inner.h[4] = b.x; K.inner.h[5] = b.y; K.inner.h[6] = b.z; K.inner.h[7] = b.w;
  K.outer.h[0] = c.x; K.outer.h[1] = c.y; K.outer.h[2] = c.z; K.outer.h[3] = c.w; K.outer.h[4] = d.x; K.outer.h[5] = d.y; K.outer.h[6] = d.z; K.outer.h[7] = d.w;
  V.h[0] = e.x; V.h[1] = e.y; V.h[2] = e.z; V.h[3] = e.w; V.h[4] = f.x; V.h[5] = f.y; V.h[6] = f.z; V.h[7] = f.w;
}
// the candidate T (= V) of step h.2 with its verdict: k = T where it is in [1, n - 1] (and the key was), else 0; ok and retry as bytes
ECS_DEV void candidate_out(const sha256_state& V, const fe& N, uint32_t key_ok, uint64_t* __restrict__ kv, retry_byte* again, uint8_t* __restrict__ okv, size_t i) {
  fe T = sha_digest_fe(V);
  const uint32_t good = in_range_mask(T, N) & key_ok;
#pragma unroll
  for (int q = 0; q < 8; ++q) T.w[q] &= good;
  fe_store(kv, i, T);
  okv[i] = (uint8_t)(good & 1u);
  *again = (uint8_t)(~good & key_ok & 1u);                     // THE declassified bit (a key out of range never retries: its lane is refused)
}

__global__ void __launch_bounds__(BLOCK) k_rfc6979_first(words8 order, const uint64_t* __restrict__ ev, const uint64_t* __restrict__ dv, uint64_t* __restrict__ kv,
                                                         uint4* __restrict__ state, uint8_t* __restrict__ retry, uint8_t* __restrict__ okv, size_t n) {
  GID;
  const fe N = words8_fe(order);
  const fe e = fe_load(ev, i), d = fe_load(dv, i);
  fe red;
  const uint32_t below = sub8_3(red, e, N);                    // bits2octets(h1): e - n where e >= n
  uint32_t x[8], h1[8];
  sha_words_of(d, x);                                          // int2octets(d)
  sha_words_of(fe_select(below, e, red), h1);
  const uint32_t key_ok = in_range_mask(d, N);
  sha256_state zero_key, V;
#pragma unroll
  for (int j = 0; j < 8; ++j) { zero_key.h[j] = 0u; V.h[j] = 0x01010101u; }                  // steps b, c
  hmac_key K = hmac_key_from(zero_key);                        // constants: folded at compile time
#pragma unroll 1
  for (uint32_t sep = 0; sep < 2; ++sep) {                     // steps d, e (separator 0x00) and f, g (0x01): 7 compressions each
    K = hmac_key_from(hmac97(K, V, sep, x, h1));
    V = hmac32(K, V);
  }
  V = hmac32(K, V);                                            // step h.2: tlen = qlen after one HMAC
  state_store(state, i, K, V);
  candidate_out(V, N, key_ok, kv, (retry_byte*)(retry + i), okv, i);
}

// Lanes with retry = 0 leave at once.  The others draw further candidates until one is in range or `cap` candidates (the first included) are spent;
// the byte is written and read back through a volatile pointer: the loop's condition is the byte in memory, public data, not the register it came from.
__global__ void __launch_bounds__(BLOCK) k_rfc6979_retry(words8 order, uint64_t* __restrict__ kv, const uint4* __restrict__ state, uint8_t* retry,
                                                         uint8_t* __restrict__ okv, size_t n, uint32_t cap) {
  GID;
  retry_byte* again = (retry_byte*)(retry + i);
  if (*again == 0) return;
  const fe N = words8_fe(order);
  hmac_key K; sha256_state V;
  state_load(state, i, K, V);
  for (uint32_t tried = 1; tried < cap && *again != 0; ++tried) {
    K = hmac_key_from(hmac32_zero(K, V));                      // h.3: K = HMAC_K(V || 0x00)
    V = hmac32(K, V);                                          //      V = HMAC_K(V)
    V = hmac32(K, V);                                          // h.2 again
    candidate_out(V, N, 0xffffffffu, kv, again, okv, i);
  }
}
}  // namespace

namespace launch {
void sha256(hipStream_t s, const uint8_t* msg, size_t msg_bytes, size_t stride_bytes, uint64_t* e, size_t n) {
  const uint32_t aligned = ((reinterpret_cast<uintptr_t>(msg) | stride_bytes) & 3u) == 0 ? 1u : 0u;
  hipLaunchKernelGGL(k_sha256, grid_for(n), dim3(BLOCK), 0, s, msg, msg_bytes, stride_bytes, e, n, aligned);
}
void rfc6979_nonce(hipStream_t s, const words8& order, const uint64_t* e, const uint64_t* d, uint64_t* k, void* state, uint8_t* retry, uint8_t* ok, size_t n, unsigned cap) {
  hipLaunchKernelGGL(k_rfc6979_first, grid_for(n), dim3(BLOCK), 0, s, order, e, d, k, static_cast<uint4*>(state), retry, ok, n);
  hipLaunchKernelGGL(k_rfc6979_retry, grid_for(n), dim3(BLOCK), 0, s, order, k, static_cast<const uint4*>(state), retry, ok, n, (uint32_t)cap);
}
}  // namespace launch
}  // namespace ecsimd_hip
