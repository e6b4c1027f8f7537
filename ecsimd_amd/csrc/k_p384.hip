// k_p384.hip -- NIST P-384: the kernels behind ecsimd_p384_sha384 / _pubkey / _ecdh / _ecdsa_verify / _ecdsa_sign / _raw (include/ecsimd_p384.h).
// fe384.cuh is the field and the scalars modulo n, p384.cuh the complete group law and the three window loops, sha512.cuh the compression (SHA-384 is its
// other IV and 48 bytes out).  One lane per element; integers are 48 big-endian bytes at any alignment (word accesses where an array's base is a multiple
// of 4: one flag per array).
//
// SECRET data -- selects by masks only; no branch, address or lane mask made of d, k, the HMAC states, e + r d or a point on the way; nothing declassified;
// no scratch memory (tools/ct_check.py check_secret_flow and tests/test_p384_cpu.py hold the ISA to that):
//   * k_p384_pubkey        pub = d G by the comb, one inversion; ok = 1 <= d < n, zeros where not.
//   * k_p384_ecdh          z = x(d peer): the lane's table of 1 .. 8 peer into the workspace, the signed 4-bit window loop, one inversion;
//                          ok = 1 <= d < n and the peer decodes, zeros where not.
//   * k_p384_sign_nonce    k = the first RFC 6979 candidate (HMAC-SHA-384 over d and the digest), into the workspace with valid = 1 <= d, k < n.
//   * k_p384_sign_finish   R = k G by the comb, r = x(R) mod n, s = (e + r d) / k mod n; ok = valid, r != 0, s != 0; zeros where not.
// PUBLIC data (the same masked code):
//   * k_p384_sha384        SHA-384 of each lane's message (lengths may differ per lane).
//   * k_p384_verify        1 <= r, s < n, pub decodes, u1 G + u2 Q by one Straus loop is not the identity and x(R) = r modulo n (projectively).
//   * k_p384_raw           one function of the layers below on raw operands (ecsimd_p384_raw).
#include "kernels.h"
#include "sha512.cuh"
#include "p384.cuh"

namespace ecsimd_hip {
namespace {
using launch::BLOCK;
#define GID size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x; if (i >= n) return

// ---- SHA-384
ECS_DEV sha512_state sha384_iv() {
  sha512_state s;
  s.h[0] = 0xcbbb9d5dc1059ed8ull; s.h[1] = 0x629a292a367cd507ull; s.h[2] = 0x9159015a3070dd17ull; s.h[3] = 0x152fecd8f70e5939ull;
  s.h[4] = 0x67332667ffc00b31ull; s.h[5] = 0x8eb44a8768581511ull; s.h[6] = 0xdb0c2e0d64f98fa7ull; s.h[7] = 0x47b5481dbefa4fa4ull;
  return s;
}
// digest bytes 0 .. 47 as the big-endian integer they spell, and back to the six big-endian words
ECS_DEV fe384 sha384_digest_int(const sha512_state& s) {
  fe384 r;
#pragma unroll
  for (int j = 0; j < 6; ++j) { r.w[11 - 2 * j] = (uint32_t)(s.h[j] >> 32); r.w[10 - 2 * j] = (uint32_t)s.h[j]; }
  return r;
}
ECS_DEV void p384_be_words(const fe384& x, uint64_t (&be)[6]) {
#pragma unroll
  for (int j = 0; j < 6; ++j) be[j] = sha512_join(x.w[11 - 2 * j], x.w[10 - 2 * j]);
}
// SHA-384 of the len bytes at p: whole 64-bit words are word loads while they lie inside the message, the word it ends in byte loads; len is PUBLIC and
// alone decides the trip count and every load
ECS_DEV sha512_state sha384_message(const uint8_t* __restrict__ p, size_t len, uint32_t aligned) {
  sha512_state s = sha384_iv();
  const size_t blocks = (len + 17 + 127) / 128;
#pragma unroll 1
  for (size_t b = 0; b < blocks; ++b) {
    sha512_block m;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      uint64_t w = 0;
      const size_t off = 128 * b + 8 * j;
      if (off + 8 <= len) {
        if (aligned) {
          const uint32_t* q = reinterpret_cast<const uint32_t*>(p + off);
          w = sha512_join(__builtin_bswap32(q[0]), __builtin_bswap32(q[1]));
        } else {
#pragma unroll
          for (int t = 0; t < 8; ++t) w = (w << 8) | (uint64_t)p[off + t];
        }
      } else if (off <= len) {
#pragma unroll
        for (int t = 0; t < 8; ++t) {
          uint64_t byte = 0;
          if (off + t < len) byte = p[off + t];
          else if (off + t == len) byte = 0x80u;
          w = (w << 8) | byte;
        }
      }
      m.w[j] = w;
    }
    if (b + 1 == blocks) m.w[15] = (uint64_t)len * 8u;
    sha512_compress(s, m);
  }
  return s;
}
__global__ void __launch_bounds__(BLOCK) k_p384_sha384(const uint8_t* __restrict__ msg, size_t msg_bytes, size_t stride, const uint32_t* __restrict__ lens, uint32_t aligned,
                                                       uint8_t* __restrict__ digest, uint32_t digest_aligned, size_t n) {
  GID;
  size_t len = msg_bytes;
  if (lens) { len = lens[i]; len = len < stride ? len : stride; }
  p384_store48(digest + 48 * i, sha384_digest_int(sha384_message(msg + i * stride, len, aligned)), digest_aligned);
}

// ---- HMAC-SHA-384 with a 48-byte key, as RFC 6979 uses it (secret data)
struct hmac384_key { sha512_state inner, outer; };
ECS_DEV hmac384_key hmac384_key_from(const uint64_t (&key)[6]) {
  sha512_block bi, bo;
#pragma unroll
  for (int j = 0; j < 16; ++j) { const uint64_t k = j < 6 ? key[j < 6 ? j : 0] : 0ull; bi.w[j] = k ^ 0x3636363636363636ull; bo.w[j] = k ^ 0x5c5c5c5c5c5c5c5cull; }
  hmac384_key k;
  k.inner = sha384_iv(); sha512_compress(k.inner, bi);
  k.outer = sha384_iv(); sha512_compress(k.outer, bo);
  return k;
}
// the last block of a hash of 128 + 48 bytes whose final 48 are v
ECS_DEV sha512_block sha384_tail48(const uint64_t (&v)[6]) {
  sha512_block b;
#pragma unroll
  for (int j = 0; j < 6; ++j) b.w[j] = v[j];
  b.w[6] = 0x8000000000000000ull;
#pragma unroll
  for (int j = 7; j < 15; ++j) b.w[j] = 0u;
  b.w[15] = (128ull + 48ull) * 8u;
  return b;
}
ECS_DEV void hmac384_finish(const hmac384_key& k, const sha512_state& inner, uint64_t (&out)[6]) {
  uint64_t d[6];
#pragma unroll
  for (int j = 0; j < 6; ++j) d[j] = inner.h[j];
  sha512_state o = k.outer;
  sha512_compress(o, sha384_tail48(d));
#pragma unroll
  for (int j = 0; j < 6; ++j) out[j] = o.h[j];
}
// V = HMAC_K(V)
ECS_DEV void hmac384_v(const hmac384_key& k, uint64_t (&V)[6]) {
  sha512_state in = k.inner;
  sha512_compress(in, sha384_tail48(V));
  hmac384_finish(k, in, V);
}
// K = HMAC_K(V || sep || x || h): 145 bytes behind the key block.  x and h sit one byte off the word grid: D_j = (the last byte of the word before) : (seven
// bytes of this one).
ECS_DEV void hmac384_k(const hmac384_key& k, const uint64_t (&V)[6], uint32_t sep, const uint64_t (&x)[6], const uint64_t (&h)[6], uint64_t (&K)[6]) {
  uint64_t s[13];                                             // sep || x || h || 0x80, as words
  s[0] = ((uint64_t)sep << 56) | (x[0] >> 8);
#pragma unroll
  for (int j = 1; j < 6; ++j) s[j] = (x[j - 1] << 56) | (x[j] >> 8);
  s[6] = (x[5] << 56) | (h[0] >> 8);
#pragma unroll
  for (int j = 1; j < 6; ++j) s[6 + j] = (h[j - 1] << 56) | (h[j] >> 8);
  s[12] = (h[5] << 56) | (0x80ull << 48);
  sha512_state in = k.inner;
  sha512_block b;
#pragma unroll
  for (int j = 0; j < 6; ++j) b.w[j] = V[j];
#pragma unroll
  for (int j = 0; j < 10; ++j) b.w[6 + j] = s[j];
  sha512_compress(in, b);
  b.w[0] = s[10]; b.w[1] = s[11]; b.w[2] = s[12];
#pragma unroll
  for (int j = 3; j < 15; ++j) b.w[j] = 0u;
  b.w[15] = (128ull + 145ull) * 8u;
  sha512_compress(in, b);
  hmac384_finish(k, in, K);
}

// ---- the secret kernels
__global__ void __launch_bounds__(BLOCK) k_p384_pubkey(const uint8_t* __restrict__ d, uint32_t d_aligned, uint8_t* __restrict__ pub, uint32_t pub_aligned,
                                                       uint8_t* __restrict__ ok, size_t n) {
  GID;
  const fe384 k = p384_load48(d + 48 * i, d_aligned);
  const uint32_t good = sc384_in_range(k);
  const p384_affine a = p384_to_affine(p384_base_ct(k, P384_BASE));
  const fe384 zero = fe384_small(0u);
  p384_store48(pub + 96 * i, fe384_select(good, a.x, zero), pub_aligned);
  p384_store48(pub + 96 * i + 48, fe384_select(good, a.y, zero), pub_aligned);
  ok[i] = (uint8_t)(good & 1u);
}
__global__ void __launch_bounds__(BLOCK) k_p384_ecdh(const uint8_t* __restrict__ d, uint32_t d_aligned, const uint8_t* __restrict__ peer, uint32_t peer_aligned,
                                                     uint32_t* __restrict__ table, uint8_t* __restrict__ z, uint32_t z_aligned, uint8_t* __restrict__ ok, size_t n) {
  GID;
  const fe384 k = p384_load48(d + 48 * i, d_aligned);
  const p384_affine q = {p384_load48(peer + 96 * i, peer_aligned), p384_load48(peer + 96 * i + 48, peer_aligned)};
  const uint32_t good = sc384_in_range(k) & p384_valid(q);
  p384_table_build(table, n, i, p384_from_affine({fe384_canon(q.x), fe384_canon(q.y)}));
  const p384_point r = p384_var_ct(k, table, n, i);
  const fe384 x = fe384_mul(r.X, fe384_invert(r.Z));
  p384_store48(z + 48 * i, fe384_select(good, x, fe384_small(0u)), z_aligned);
  ok[i] = (uint8_t)(good & 1u);
}
// kws: word-major, twelve words of k and one of valid per lane (kws[w * n + i])
__global__ void __launch_bounds__(BLOCK) k_p384_sign_nonce(const uint8_t* __restrict__ d, uint32_t d_aligned, const uint8_t* __restrict__ digest, uint32_t digest_aligned,
                                                           uint32_t* __restrict__ kws, size_t n) {
  GID;
  const fe384 x = p384_load48(d + 48 * i, d_aligned);
  const fe384 h1 = sc384_reduce(p384_load48(digest + 48 * i, digest_aligned));   // bits2octets: hlen = qlen, one conditional subtraction
  uint64_t xw[6], hw[6], K[6], V[6];
  p384_be_words(x, xw); p384_be_words(h1, hw);
#pragma unroll
  for (int j = 0; j < 6; ++j) { K[j] = 0ull; V[j] = 0x0101010101010101ull; }
  hmac384_key key;
#pragma unroll 1
  for (uint32_t sep = 0; sep < 2; ++sep) {
    key = hmac384_key_from(K);
    hmac384_k(key, V, sep, xw, hw, K);
    key = hmac384_key_from(K);
    hmac384_v(key, V);
  }
  hmac384_v(key, V);                                            // the first candidate; 2^384 - n < 2^190: out of range with probability below 2^-194
  fe384 k;
#pragma unroll
  for (int j = 0; j < 6; ++j) { k.w[11 - 2 * j] = (uint32_t)(V[j] >> 32); k.w[10 - 2 * j] = (uint32_t)V[j]; }
  const uint32_t good = sc384_in_range(x) & sc384_in_range(k);
#pragma unroll
  for (int q = 0; q < 12; ++q) kws[(size_t)q * n + i] = k.w[q] & good;
  kws[(size_t)12 * n + i] = good;
}
__global__ void __launch_bounds__(BLOCK) k_p384_sign_finish(const uint8_t* __restrict__ d, uint32_t d_aligned, const uint8_t* __restrict__ digest, uint32_t digest_aligned,
                                                            const uint32_t* __restrict__ kws, uint8_t* __restrict__ sig, uint32_t sig_aligned, uint8_t* __restrict__ ok, size_t n) {
  GID;
  fe384 k;
#pragma unroll
  for (int q = 0; q < 12; ++q) k.w[q] = kws[(size_t)q * n + i];
  uint32_t good = kws[(size_t)12 * n + i];
  const p384_point R = p384_base_ct(k, P384_BASE);
  const fe384 r = sc384_reduce(fe384_mul(R.X, fe384_invert(R.Z)));
  const fe384 x = sc384_reduce(p384_load48(d + 48 * i, d_aligned));
  const fe384 e = sc384_reduce(p384_load48(digest + 48 * i, digest_aligned));
  const fe384 s = sc384_mul(sc384_invert(k), sc384_add(e, sc384_mul(r, x)));
  good &= ~fe384_is_zero(r) & ~fe384_is_zero(s);
  const fe384 zero = fe384_small(0u);
  p384_store48(sig + 96 * i, fe384_select(good, r, zero), sig_aligned);
  p384_store48(sig + 96 * i + 48, fe384_select(good, s, zero), sig_aligned);
  ok[i] = (uint8_t)(good & 1u);
}

// ---- verification (public data)
__global__ void __launch_bounds__(BLOCK) k_p384_verify(const uint8_t* __restrict__ pub, uint32_t pub_aligned, const uint8_t* __restrict__ digest, uint32_t digest_aligned,
                                                       const uint8_t* __restrict__ sig, uint32_t sig_aligned, uint32_t* __restrict__ table, uint8_t* __restrict__ ok, size_t n) {
  GID;
  const p384_affine q = {p384_load48(pub + 96 * i, pub_aligned), p384_load48(pub + 96 * i + 48, pub_aligned)};
  const fe384 r = p384_load48(sig + 96 * i, sig_aligned), s = p384_load48(sig + 96 * i + 48, sig_aligned);
  const uint32_t good = sc384_in_range(r) & sc384_in_range(s) & p384_valid(q);
  const fe384 e = sc384_reduce(p384_load48(digest + 48 * i, digest_aligned));
  const fe384 w = sc384_invert(sc384_reduce(s));
  const fe384 u1 = sc384_mul(e, w), u2 = sc384_mul(sc384_reduce(r), w);
  p384_table_build(table, n, i, p384_from_affine({fe384_canon(q.x), fe384_canon(q.y)}));
  const p384_point R = p384_double_mult(u1, u2, P384_BASE, table, n, i);
  ok[i] = (uint8_t)(good & p384_x_equals_mod_n(R, sc384_reduce(r)) & 1u);
}

// ---- one function of the layers on raw 48-byte records (launch::p384_raw_inputs / _outputs of them per lane)
__global__ void __launch_bounds__(BLOCK) k_p384_raw(int op, const uint8_t* __restrict__ in, uint8_t* __restrict__ out, uint32_t aligned, uint32_t* __restrict__ table, size_t n) {
  GID;
  const int ni = launch::p384_raw_inputs(op), no = launch::p384_raw_outputs(op);
  const uint8_t* ip = in + (size_t)48 * ni * i;
  uint8_t* op_ = out + (size_t)48 * no * i;
  fe384 a[6];
#pragma unroll
  for (int j = 0; j < 6; ++j) a[j] = j < ni ? p384_load48(ip + 48 * j, aligned) : fe384_small(0u);
  fe384 r = fe384_small(0u);
  p384_point pt = p384_identity();
  if (op <= launch::P384_RAW_SC_INVERT) {
    const fe384 x = fe384_canon(a[0]), y = fe384_canon(a[1]);
    switch (op) {
      case launch::P384_RAW_FE_MUL: r = fe384_mul(x, y); break;
      case launch::P384_RAW_FE_SQR: r = fe384_sqr(x); break;
      case launch::P384_RAW_FE_ADD: r = fe384_add(x, y); break;
      case launch::P384_RAW_FE_SUB: r = fe384_sub(x, y); break;
      case launch::P384_RAW_FE_NEG: r = fe384_neg(x); break;
      case launch::P384_RAW_FE_INVERT: r = fe384_invert(x); break;
      case launch::P384_RAW_FE_CANON: r = x; break;
      case launch::P384_RAW_SC_MUL: r = sc384_mul(sc384_reduce(a[0]), sc384_reduce(a[1])); break;
      default: r = sc384_invert(sc384_reduce(a[0])); break;
    }
    p384_store48(op_, r, aligned);
    return;
  }
  uint32_t flag = 0;                                           // DECODE_ENCODE: the point decodes; the others: the result is the identity
  switch (op) {
    case launch::P384_RAW_DECODE_ENCODE: {
      flag = p384_valid({a[0], a[1]});
      pt = p384_select(flag, p384_from_affine({fe384_canon(a[0]), fe384_canon(a[1])}), pt);
      break; }
    case launch::P384_RAW_POINT_ADD: {
      const p384_point p1 = p384_select(0u - (a[2].w[0] & 1u), p384_identity(), p384_from_affine({fe384_canon(a[0]), fe384_canon(a[1])}));
      const p384_point p2 = p384_select(0u - (a[5].w[0] & 1u), p384_identity(), p384_from_affine({fe384_canon(a[3]), fe384_canon(a[4])}));
      pt = p384_add(p1, p2);
      break; }
    case launch::P384_RAW_POINT_DBL:
      pt = p384_dbl(p384_select(0u - (a[2].w[0] & 1u), p384_identity(), p384_from_affine({fe384_canon(a[0]), fe384_canon(a[1])})));
      break;
    case launch::P384_RAW_BASE_MULT: pt = p384_base_ct(sc384_reduce(a[0]), P384_BASE); break;
    case launch::P384_RAW_VAR_MULT:
      p384_table_build(table, n, i, p384_from_affine({fe384_canon(a[1]), fe384_canon(a[2])}));
      pt = p384_var_ct(sc384_reduce(a[0]), table, n, i);
      break;
    default:
      p384_table_build(table, n, i, p384_from_affine({fe384_canon(a[2]), fe384_canon(a[3])}));
      pt = p384_double_mult(sc384_reduce(a[0]), sc384_reduce(a[1]), P384_BASE, table, n, i);
      break;
  }
  const p384_affine q = p384_to_affine(pt);
  if (op != launch::P384_RAW_DECODE_ENCODE) flag = p384_is_identity(pt);
  p384_store48(op_, q.x, aligned);
  p384_store48(op_ + 48, q.y, aligned);
  p384_store48(op_ + 96, fe384_small(flag & 1u), aligned);
}
}  // namespace

namespace launch {
static uint32_t word_aligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0 ? 1u : 0u; }
void p384_sha384(hipStream_t s, const uint8_t* msg, size_t msg_bytes, size_t stride_bytes, const uint32_t* lens, uint8_t* digest, size_t n) {
  const uint32_t aligned = word_aligned(msg) & ((stride_bytes & 3u) == 0 ? 1u : 0u);
  hipLaunchKernelGGL(k_p384_sha384, grid_for(n), dim3(BLOCK), 0, s, msg, msg_bytes, stride_bytes, lens, aligned, digest, word_aligned(digest), n);
}
void p384_pubkey(hipStream_t s, const uint8_t* d, uint8_t* pub, uint8_t* ok, size_t n) {
  hipLaunchKernelGGL(k_p384_pubkey, grid_for(n), dim3(BLOCK), 0, s, d, word_aligned(d), pub, word_aligned(pub), ok, n);
}
void p384_ecdh(hipStream_t s, const uint8_t* d, const uint8_t* peer, uint32_t* table, uint8_t* z, uint8_t* ok, size_t n) {
  hipLaunchKernelGGL(k_p384_ecdh, grid_for(n), dim3(BLOCK), 0, s, d, word_aligned(d), peer, word_aligned(peer), table, z, word_aligned(z), ok, n);
}
void p384_sign_nonce(hipStream_t s, const uint8_t* d, const uint8_t* digest, uint32_t* kws, size_t n) {
  hipLaunchKernelGGL(k_p384_sign_nonce, grid_for(n), dim3(BLOCK), 0, s, d, word_aligned(d), digest, word_aligned(digest), kws, n);
}
void p384_sign_finish(hipStream_t s, const uint8_t* d, const uint8_t* digest, const uint32_t* kws, uint8_t* sig, uint8_t* ok, size_t n) {
  hipLaunchKernelGGL(k_p384_sign_finish, grid_for(n), dim3(BLOCK), 0, s, d, word_aligned(d), digest, word_aligned(digest), kws, sig, word_aligned(sig), ok, n);
}
void p384_verify(hipStream_t s, const uint8_t* pub, const uint8_t* digest, const uint8_t* sig, uint32_t* table, uint8_t* ok, size_t n) {
  hipLaunchKernelGGL(k_p384_verify, grid_for(n), dim3(BLOCK), 0, s, pub, word_aligned(pub), digest, word_aligned(digest), sig, word_aligned(sig), table, ok, n);
}
void p384_raw(hipStream_t s, int op, const uint8_t* in, uint8_t* out, uint32_t* table, size_t n) {
  hipLaunchKernelGGL(k_p384_raw, grid_for(n), dim3(BLOCK), 0, s, op, in, out, word_aligned(in) & word_aligned(out), table, n);
}
}  // namespace launch
}  // namespace ecsimd_hip
