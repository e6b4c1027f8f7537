// k_sm2.hip -- the SM2 signature scheme (GB/T 32918.2, ISO/IEC 14888-3) around the generic curve kernels: the SM3 hash (sm3.cuh), the identity digest Z_A,
// the message digest e, and the scalar-field halves of verification and signing.  The point arithmetic is k_gcomb.hip's and k_gvarwin.hip's, unchanged.
//
//   * k_sm3                  SM3 of one message per lane; equal lengths or one length per lane.  Public data.
//   * k_sm2_za               Z_A = SM3(ENTL || ID || a || b || x_G || y_G || x_A || y_A).  Public data.
//   * k_sm2_digest           e = SM3(Z_A || M), Z_A made in registers and never written.  Public data.
//   * k_sm2_verify_scalars   valid = 1 <= r, s < n and t != 0 with t = (r + s) mod n; u1 = s, u2 = t (zeros where not valid).  Public data.
//   * k_sm2_accept           ok = valid and finite and (e mod n + x(R) mod n) mod n == r.  Public data.
//   * k_sm2_sign_scalars     r = (e + x(k G)) mod n, s = (1 + d)^-1 (k - r d) mod n for SECRET d and k.
//   * k_sm2_key_range        ok = 1 <= d <= n - 2 for the SECRET d of pubkey; the point is zeroed where not.
//
// Secrets: d, k and everything made of them.  The two kernels that see them use selects and the branch-free functions of gfield.cuh only (g_mul, g_add,
// g_sub, the division-step inversion): no branch condition, address or lane mask in force at a memory access depends on a secret
// (tools/ct_check.py check_secret_flow on the shipped ISA), and neither uses scratch memory or LDS.
#include "kernels.h"
#include "sm3.cuh"
#include "gfield.cuh"

namespace ecsimd_hip {
namespace {
using launch::BLOCK;
using launch::words8;
#define GID size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x; if (i >= n) return

ECS_DEV fe sm3_digest_fe(const sm3_state& s) {
  fe r;
#pragma unroll
  for (int j = 0; j < 8; ++j) r.w[7 - j] = s.h[j];
  return r;
}
ECS_DEV sm2_int int_of(const fe& a) {
  sm2_int r;
#pragma unroll
  for (int j = 0; j < 8; ++j) r.w[j] = a.w[j];
  return r;
}
ECS_DEV sm2_int int_of(const words8& a) {
  sm2_int r;
#pragma unroll
  for (int j = 0; j < 8; ++j) r.w[j] = a.w[j];
  return r;
}
ECS_DEV fe fe_of(const sm2_int& a) {
  fe r;
#pragma unroll
  for (int j = 0; j < 8; ++j) r.w[j] = a.w[j];
  return r;
}
// the curve's a, b, x_G, y_G and the lane's public key as the 48 big-endian words behind ENTL || ID
struct za_curve { words8 a, b, gx, gy; };
ECS_DEV sm3_state za_of(const za_curve& C, const uint64_t* __restrict__ qx, const uint64_t* __restrict__ qy, const uint8_t* __restrict__ id, uint32_t id_bytes, size_t id_stride,
                        const uint8_t* spare, size_t i) {
  const fe x = fe_load(qx, i), y = fe_load(qy, i);
  uint32_t t[48];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    t[j] = C.a.w[7 - j]; t[8 + j] = C.b.w[7 - j]; t[16 + j] = C.gx.w[7 - j]; t[24 + j] = C.gy.w[7 - j];
    t[32 + j] = x.w[7 - j]; t[40 + j] = y.w[7 - j];
  }
  return sm3_za(id + i * id_stride, id_bytes, spare, t);
}

// msg_bytes, stride and `aligned` (the base and the stride are multiples of 4) are the same for every lane; lens == nullptr: every lane has msg_bytes bytes
__global__ void __launch_bounds__(BLOCK) k_sm3(const uint8_t* __restrict__ msg, uint32_t msg_bytes, size_t stride, const uint32_t* __restrict__ lens, uint64_t* __restrict__ out,
                                               size_t n, uint32_t aligned) {
  GID;
  const uint32_t len = lens ? lens[i] : msg_bytes;
  const uint8_t* spare = reinterpret_cast<const uint8_t*>(out + 4 * i);
  sm3_state s = sm3_iv();
  if (aligned) sm3_absorb_message<true>(s, msg + i * stride, len, spare);
  else sm3_absorb_message<false>(s, msg + i * stride, len, spare);
  fe_store(out, i, sm3_digest_fe(s));
}

__global__ void __launch_bounds__(BLOCK) k_sm2_za(za_curve C, const uint64_t* __restrict__ qx, const uint64_t* __restrict__ qy, const uint8_t* __restrict__ id, uint32_t id_bytes,
                                                  size_t id_stride, uint64_t* __restrict__ out, size_t n) {
  GID;
  const sm3_state z = za_of(C, qx, qy, id, id_bytes, id_stride, reinterpret_cast<const uint8_t*>(out + 4 * i), i);
  fe_store(out, i, sm3_digest_fe(z));
}

__global__ void __launch_bounds__(BLOCK) k_sm2_digest(za_curve C, const uint64_t* __restrict__ qx, const uint64_t* __restrict__ qy, const uint8_t* __restrict__ id, uint32_t id_bytes,
                                                      size_t id_stride, const uint8_t* __restrict__ msg, uint32_t msg_bytes, size_t stride, const uint32_t* __restrict__ lens,
                                                      uint64_t* __restrict__ out, size_t n, uint32_t aligned) {
  GID;
  const uint8_t* spare = reinterpret_cast<const uint8_t*>(out + 4 * i);
  const sm3_state z = za_of(C, qx, qy, id, id_bytes, id_stride, spare, i);
  const uint32_t len = lens ? lens[i] : msg_bytes;
  sm3_state s = sm3_iv();
  if (aligned) sm3_absorb_after32<true>(s, z.h, msg + i * stride, len, spare);
  else sm3_absorb_after32<false>(s, z.h, msg + i * stride, len, spare);
  fe_store(out, i, sm3_digest_fe(s));
}

__global__ void __launch_bounds__(BLOCK) k_sm2_verify_scalars(words8 order, const uint64_t* __restrict__ rv, const uint64_t* __restrict__ sv, uint64_t* __restrict__ u1,
                                                              uint64_t* __restrict__ u2, uint8_t* __restrict__ valid, size_t n) {
  GID;
  sm2_int a, b;
  valid[i] = (uint8_t)sm2_verify_scalars(int_of(fe_load(rv, i)), int_of(fe_load(sv, i)), int_of(order), a, b);
  fe_store(u1, i, fe_of(a));
  fe_store(u2, i, fe_of(b));
}

__global__ void __launch_bounds__(BLOCK) k_sm2_accept(words8 order, const uint64_t* __restrict__ ev, const uint64_t* __restrict__ xv, const uint8_t* __restrict__ finite,
                                                      const uint64_t* __restrict__ rv, const uint8_t* __restrict__ valid, uint8_t* __restrict__ ok, size_t n) {
  GID;
  const uint32_t same = sm2_accept(int_of(fe_load(ev, i)), int_of(fe_load(xv, i)), int_of(fe_load(rv, i)), int_of(order));
  ok[i] = (uint8_t)(same & (uint32_t)(valid[i] != 0) & (uint32_t)(finite[i] != 0));
}

// all ones where 1 <= v < n, as data
ECS_DEV uint32_t in_range_mask(const fe& v, const fe& N) {
  fe t;
  return sub8_3(t, v, N) & ~g_zero_mask(v);
}
ECS_DEV fe fe_one() {
  fe one;
#pragma unroll
  for (int j = 0; j < 8; ++j) one.w[j] = (j == 0) ? 1u : 0u;
  return one;
}
// all ones where 1 <= d <= n - 2: d is in [1, n - 1] and d + 1 is not n
ECS_DEV uint32_t key_range_mask(const fe& d, const fe& N, const gmod& M, fe& d1) {
  d1 = g_add(d, fe_one(), M);                                  // (1 + d) mod n where d < n
  return in_range_mask(d, N) & ~g_zero_mask(d1);
}

// SM2 signing, the arithmetic modulo the group order (GB/T 32918.2 6.1 A3 - A6; M = n's gmod): given the digest e (ANY 256-bit value), the private key d,
// the nonce k and x = x(k G) (classical, < p < 2n),
//   r = (e + x) mod n,   s = (1 + d)^-1 (k - r d) mod n,   ok = 1 <= d <= n - 2  and  1 <= k <= n - 1  and  r != 0  and  r + k != n  and  s != 0
// (r = s = 0 where not ok: a new nonce is the caller's).  d and k are SECRETS: selects and gfield.cuh's branch-free functions only.  One division-step
// inversion per lane for its m elements, shared exactly as k_ecdsa_sign_scalars shares k's (k_ecdsa_scalars has the algebra): here the running product is
// over 1 + d, an element with a bad d enters it as 1, and s[] carries the prefix products on the way up.  Seven Montgomery products per signature.
__global__ void __launch_bounds__(256) k_sm2_sign_scalars(gmod M, const uint64_t* __restrict__ ev, const uint64_t* __restrict__ dv, const uint64_t* __restrict__ kv,
                                                          const uint64_t* __restrict__ xv, uint64_t* __restrict__ rv, uint64_t* __restrict__ sv,
                                                          uint8_t* __restrict__ okv, size_t n, size_t lanes, int m) {
  const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= lanes) return;
  const fe N = g_words(M.p), one = fe_one();
  fe acc = one;
  for (int j = 0; j < m; ++j) {
    const size_t e = (size_t)j * lanes + g;
    if (e >= n) break;                                     // (a bound on the public batch length)
    fe d1;
    const uint32_t good = key_range_mask(fe_load(dv, e), N, M, d1);
    const fe dd = fe_select(good, d1, one);
    acc = (j == 0) ? dd : g_mul(acc, dd, M);               // acc_0 = (1 + d_0), acc_j = acc_(j-1) (1 + d_j) / R
    fe_store(sv, e, acc);
  }
  fe inv = g_inverse_plain(acc, M);
  int last = m - 1;
  while (last >= 0 && (size_t)last * lanes + g >= n) --last;
  const fe rsq = g_words(M.rsq);
  for (int j = last; j >= 0; --j) {
    const size_t e = (size_t)j * lanes + g;
    const fe k = fe_load(kv, e), d = fe_load(dv, e);
    fe d1;
    const uint32_t good_d = key_range_mask(d, N, M, d1);
    const fe dd = fe_select(good_d, d1, one);
    fe w;
    if (j > 0) { w = g_mul(inv, fe_load(sv, (size_t)(j - 1) * lanes + g), M); inv = g_mul(inv, dd, M); }
    else w = inv;                                          // (1 + d)^-1, plain
    fe x = fe_load(xv, e);
    g_cond_sub(x, 0, M);                                   // x < p < 2n: one conditional subtraction reduces it
    fe em = fe_load(ev, e);
    g_cond_sub(em, 0, M);                                  // e < 2^256 < 2n
    fe r = g_add(em, x, M);
    const fe rd = g_mul(g_mul(r, d, M), rsq, M);           // r d mod n
    const fe t = g_sub(k, rd, M);                          // k < n where it counts
    fe s = g_mul(g_mul(w, rsq, M), t, M);                  // ((1 + d)^-1 R) t / R
    const uint32_t ok = good_d & in_range_mask(k, N) & ~g_zero_mask(r) & ~g_zero_mask(g_add(r, k, M)) & ~g_zero_mask(s);
#pragma unroll
    for (int q = 0; q < 8; ++q) { r.w[q] &= ok; s.w[q] &= ok; }
    fe_store(rv, e, r); fe_store(sv, e, s);
    okv[e] = (uint8_t)(ok & 1u);
  }
}

// pubkey's range rule on top of the comb's d G (which reduces d modulo n): ok = 1 <= d <= n - 2 -- n - 1 is refused because 1 + d must be invertible --
// and (0, 0) where not.  SECRET d: a mask and ands.
__global__ void __launch_bounds__(BLOCK) k_sm2_key_range(gmod M, const uint64_t* __restrict__ dv, uint64_t* __restrict__ qx, uint64_t* __restrict__ qy, uint8_t* __restrict__ okv,
                                                         size_t n) {
  GID;
  fe d1;
  const uint32_t good = key_range_mask(fe_load(dv, i), g_words(M.p), M, d1);
  fe x = fe_load(qx, i), y = fe_load(qy, i);
#pragma unroll
  for (int q = 0; q < 8; ++q) { x.w[q] &= good; y.w[q] &= good; }
  fe_store(qx, i, x); fe_store(qy, i, y);
  okv[i] = (uint8_t)(good & 1u);
}
}  // namespace

namespace launch {
static uint32_t word_aligned(const void* p, size_t stride) { return ((reinterpret_cast<uintptr_t>(p) | stride) & 3u) == 0 ? 1u : 0u; }
static za_curve za_curve_of(const sm2_curve_words& c) { return {c.a, c.b, c.gx, c.gy}; }
void sm3(hipStream_t s, const uint8_t* msg, size_t msg_bytes, size_t stride_bytes, const uint32_t* lens, uint64_t* e, size_t n) {
  hipLaunchKernelGGL(k_sm3, grid_for(n), dim3(BLOCK), 0, s, msg, (uint32_t)msg_bytes, stride_bytes, lens, e, n, word_aligned(msg, stride_bytes));
}
void sm2_za(hipStream_t s, const sm2_curve_words& c, const uint64_t* qx, const uint64_t* qy, const uint8_t* id, size_t id_bytes, size_t id_stride, uint64_t* za, size_t n) {
  hipLaunchKernelGGL(k_sm2_za, grid_for(n), dim3(BLOCK), 0, s, za_curve_of(c), qx, qy, id, (uint32_t)id_bytes, id_stride, za, n);
}
void sm2_digest(hipStream_t s, const sm2_curve_words& c, const uint64_t* qx, const uint64_t* qy, const uint8_t* id, size_t id_bytes, size_t id_stride, const uint8_t* msg,
                size_t msg_bytes, size_t stride_bytes, const uint32_t* lens, uint64_t* e, size_t n) {
  hipLaunchKernelGGL(k_sm2_digest, grid_for(n), dim3(BLOCK), 0, s, za_curve_of(c), qx, qy, id, (uint32_t)id_bytes, id_stride, msg, (uint32_t)msg_bytes, stride_bytes, lens, e, n,
                     word_aligned(msg, stride_bytes));
}
void sm2_verify_scalars(hipStream_t s, const words8& order, const uint64_t* r, const uint64_t* sg, uint64_t* u1, uint64_t* u2, uint8_t* valid, size_t n) {
  hipLaunchKernelGGL(k_sm2_verify_scalars, grid_for(n), dim3(BLOCK), 0, s, order, r, sg, u1, u2, valid, n);
}
void sm2_accept(hipStream_t s, const words8& order, const uint64_t* e, const uint64_t* x, const uint8_t* finite, const uint64_t* r, const uint8_t* valid, uint8_t* ok, size_t n) {
  hipLaunchKernelGGL(k_sm2_accept, grid_for(n), dim3(BLOCK), 0, s, order, e, x, finite, r, valid, ok, n);
}
// the lanes of the shared inversion, as k_gfield.hip shapes ecdsa_sign_scalars: m = n / 2^17 elements per lane, 1 .. 128
void sm2_sign_scalars(hipStream_t s, const gmod& M, const uint64_t* e, const uint64_t* d, const uint64_t* k, const uint64_t* x, uint64_t* r, uint64_t* sg, uint8_t* ok, size_t n) {
  size_t m = n >> 17; if (m < 1) m = 1; if (m > 128) m = 128;
  const size_t lanes = (n + m - 1) / m;
  hipLaunchKernelGGL(k_sm2_sign_scalars, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, s, M, e, d, k, x, r, sg, ok, n, lanes, (int)m);
}
void sm2_key_range(hipStream_t s, const gmod& M, const uint64_t* d, uint64_t* qx, uint64_t* qy, uint8_t* ok, size_t n) {
  hipLaunchKernelGGL(k_sm2_key_range, grid_for(n), dim3(BLOCK), 0, s, M, d, qx, qy, ok, n);
}
}  // namespace launch
}  // namespace ecsimd_hip
