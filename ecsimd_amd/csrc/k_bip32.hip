// k_bip32.hip -- BIP-32 hierarchical key derivation on secp256k1: the master key of a seed, CKDpriv and the front and back of CKDpub.
//
// I = HMAC-SHA512(key, data) with a 32-byte (or constant) key and at most 64 bytes of data is four compressions: the key's ipad and opad blocks, ONE data block
// with its padding (sha512_tail_block_short) and the outer tail block.  I = IL || IR: IL is the tweak, IR the child's chain code.
// SECRET data (the seed, k_par, c_par, the affine k_par G, I, k_child, c_child; the index is PUBLIC): selects by masks only, no branch, address or lane mask in
// force at a memory access made of them, and no declassified bit (tools/ct_check.py check_secret_flow holds the ISA to that):
//   * k_bip32_master              I = HMAC-SHA512("Bitcoin seed", seed): the key is a constant, so its two midstates are the compile-time literals SEED_INNER and
//                                 SEED_OUTER (pinned to the model by tests/test_bip32_cpu.py) and a lane is two compressions.  seed_bytes (16 .. 64) is uniform.
//                                 k = IL, c = IR; ok = 0 and k = c = 0 where IL = 0 or IL >= n.
//   * k_bip32_ckd_priv<NEEDS_POINT>  data = 00 || ser256(k_par) || ser32(i) for i >= 2^31, serP(k_par G) || ser32(i) otherwise: the one-byte prefix shifts the 32
//                                 bytes against the word grid, so every block word is a funnel shift of two neighbours (k_btc_pubkey_hash's), and the two forms
//                                 differ by a select on bit 31 of the index.  k_child = IL + k_par mod n, c_child = IR; ok = 0 and zeros where k_par is not in
//                                 [1, n - 1], IL >= n or k_child = 0.  k_par G comes from the constant-time comb and the select-only simultaneous inversion in
//                                 front of this kernel; NEEDS_POINT = false has no point arrays and refuses every lane whose index is not hardened.
// PUBLIC data (the chain of ecsimd_hip_bip32_ckd_pub: front, the public comb t G, k_tweak_add, the simultaneous inversion, accept):
//   * k_bip32_ckd_pub_front       I = HMAC-SHA512(c_par, serP(K) || ser32(i)); t = IL, c_child = IR, valid = i < 2^31 && K on the curve && IL < n; where not valid
//                                 t = 0 and K = G, a point the addition can hold (k_tweak_front's convention).
//   * k_bip32_ckd_pub_accept      ok = valid && Z != 0; (cx, cy) = the affine sum, c_child kept, zeros where ok = 0.
#include "kernels.h"
#include "sha512.cuh"
#include "lift.cuh"

namespace ecsimd_hip {
namespace {
using launch::BLOCK;
using launch::words8;
#define GID size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x; if (i >= n) return

// The SHA-512 states after the ipad block and after the opad block of the key "Bitcoin seed"
struct bip32_consts {
  static constexpr uint64_t SEED_INNER[8] = {0x2e2af459060c1873ull, 0x7894b868dc88433aull, 0xdd1a797ef1a1933aull, 0xe6486d04fcb412a7ull,
                                             0xfbcc67b9a396caa0ull, 0xa2970b146f49b65eull, 0xfdf1daabc66f6248ull, 0x2ff99c812ada6dc3ull};
  static constexpr uint64_t SEED_OUTER[8] = {0xbbd27bac212e9dbdull, 0xdd0bc55e7e4037c1ull, 0xdfdd3d6890bd6424ull, 0x2902de663032b34cull,
                                             0xa30f8aa6f67899fcull, 0x69a566c30f88378full, 0x0500247985ecb694ull, 0xf6d70307c6b2d337ull};
};

// v mod n for v < 2^256 < 2 n: one masked subtraction
ECS_DEV fe reduce_once(const fe& v, const fe& N) {
  fe d;
  const uint32_t below = sub8_3(d, v, N);
  return fe_select(below, v, d);
}
ECS_DEV void fe_mask(fe& v, uint32_t m) {
#pragma unroll
  for (int q = 0; q < 8; ++q) v.w[q] &= m;
}

// HMAC-SHA512(c, prefix || be32(x) || ser32(index)): the 37 bytes in one block behind the key's
ECS_DEV sha512_state ckd_hmac(const fe& c, uint32_t prefix, const fe& x, uint32_t index) {
  sha512_block kb;
  uint64_t cw[4], xw[4];
  sha512_words_of(c, cw);
  sha512_words_of(x, xw);
#pragma unroll
  for (int j = 0; j < 16; ++j) kb.w[j] = j < 4 ? cw[j] : 0ull;
  const hmac512_key K = hmac512_key_from(kb);
  auto join = [](uint64_t hi, uint64_t lo) { return (hi << 56) | (lo >> 8); };
  uint64_t d[8];
  d[0] = join((uint64_t)prefix, xw[0]);
#pragma unroll
  for (int j = 1; j < 4; ++j) d[j] = join(xw[j - 1], xw[j]);
  d[4] = (xw[3] << 56) | ((uint64_t)index << 24);
  d[5] = 0u; d[6] = 0u; d[7] = 0u;
  sha512_state in = K.inner;
  sha512_compress(in, sha512_tail_block_short(d, 37u));
  return hmac512_finish(K.outer, in);
}

// seed_bytes in [16, 64] is the same on every lane
__global__ void __launch_bounds__(BLOCK) k_bip32_master(words8 order, const uint8_t* __restrict__ seed, uint32_t seed_bytes, size_t stride, uint64_t* __restrict__ kv,
                                                        uint64_t* __restrict__ cv, uint8_t* __restrict__ okv, size_t n) {
  GID;
  const fe N = w8_words(order);
  const uint8_t* p = seed + i * stride;
  // 64 byte loads without a branch: a position behind the seed reads the seed's last byte instead (always in bounds) and is masked away
  const uint32_t last = seed_bytes - 1u;
  uint64_t d[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    uint64_t w = 0;
#pragma unroll
    for (uint32_t t = 0; t < 8; ++t) {
      const uint32_t q = 8u * j + t;
      const uint32_t inside = q < seed_bytes ? 0xffu : 0u;
      w = (w << 8) | (uint64_t)(p[q < seed_bytes ? q : last] & inside);
    }
    d[j] = w;
  }
  sha512_state in, out;
#pragma unroll
  for (int j = 0; j < 8; ++j) { in.h[j] = bip32_consts::SEED_INNER[j]; out.h[j] = bip32_consts::SEED_OUTER[j]; }
  sha512_compress(in, sha512_tail_block_short(d, seed_bytes));
  const sha512_state I = hmac512_finish(out, in);
  fe k = sha512_digest_fe(I, 0), c = sha512_digest_fe(I, 4), scratch;
  const uint32_t keep = sub8_3(scratch, k, N) & ~g_zero_mask(k);                   // all ones where 1 <= IL < n
  fe_mask(k, keep); fe_mask(c, keep);
  fe_store(kv, i, k); fe_store(cv, i, c);
  okv[i] = (uint8_t)(keep & 1u);
}

// M = n's gmod.  (xP, yP) = the affine k_par G (NEEDS_POINT only).  index == NULL: every lane uses index_all.
template <bool NEEDS_POINT>
__global__ void __launch_bounds__(BLOCK) k_bip32_ckd_priv(gmod M, const uint64_t* __restrict__ kpar, const uint64_t* __restrict__ cpar, const uint32_t* __restrict__ index,
                                                          uint32_t index_all, const uint64_t* __restrict__ xPv, const uint64_t* __restrict__ yPv, uint64_t* __restrict__ kout,
                                                          uint64_t* __restrict__ cout, uint8_t* __restrict__ okv, size_t n) {
  GID;
  const fe N = g_words(M.p);
  const uint32_t idx = index ? index[i] : index_all;
  const uint32_t hardened = 0u - (idx >> 31);                                      // public
  const fe k = fe_load(kpar, i);
  fe scratch;
  uint32_t keep = sub8_3(scratch, k, N) & ~g_zero_mask(k);                         // all ones where 1 <= k_par < n
  fe x = k;
  uint32_t prefix = 0u;
  if constexpr (NEEDS_POINT) {
    x = fe_select(hardened, k, fe_load(xPv, i));
    prefix = ~hardened & (2u | ((uint32_t)yPv[4 * i] & 1u));
  } else {
    keep &= hardened;
  }
  const sha512_state I = ckd_hmac(fe_load(cpar, i), prefix, x, idx);
  fe il = sha512_digest_fe(I, 0), c = sha512_digest_fe(I, 4);
  const uint32_t il_ok = sub8_3(scratch, il, N);                                   // all ones where IL < n
  fe_mask(il, il_ok);
  fe sum = g_add(il, reduce_once(k, N), M);                                        // a refused lane's k_par may be anything: below n for g_add
  keep &= il_ok & ~g_zero_mask(sum);
  fe_mask(sum, keep); fe_mask(c, keep);
  fe_store(kout, i, sum); fe_store(cout, i, c);
  okv[i] = (uint8_t)(keep & 1u);
}

__global__ void __launch_bounds__(BLOCK) k_bip32_ckd_pub_front(words8 order, const uint64_t* __restrict__ qx, const uint64_t* __restrict__ qy, const uint64_t* __restrict__ cpar,
                                                               const uint32_t* __restrict__ index, uint32_t index_all, uint64_t* __restrict__ ox, uint64_t* __restrict__ oy,
                                                               uint64_t* __restrict__ ot, uint64_t* __restrict__ oc, uint8_t* __restrict__ valid, size_t n) {
  GID;
  constexpr int C = CURVE_SECP256K1, CI = curve_domain<C>::fast;
  const fe N = w8_words(order), P = FE_CONST(C, P);
  const uint32_t idx = index ? index[i] : index_all;
  fe x = fe_load(qx, i), y = fe_load(qy, i);
  bool ok = idx < 0x80000000u && g_less(x, P) && g_less(y, P);
  const fe xm = classical_to_fast<C>(x), ym = classical_to_fast<C>(y);
  ok = ok && fe_eq(fe_sqr<CI>(ym), fe_add<CI>(fe_mul<CI>(fe_sqr<CI>(xm), xm), FE_CONST(CI, BM)));   // y^2 = x^3 + 7
  const sha512_state I = ckd_hmac(fe_load(cpar, i), 2u | (y.w[0] & 1u), x, idx);
  fe t = sha512_digest_fe(I, 0), c = sha512_digest_fe(I, 4);
  ok = ok && g_less(t, N);
  if (!ok) { x = FE_CONST(C, GX); y = FE_CONST(C, GY); t = fe_zero(); c = fe_zero(); }
  fe_store(ox, i, x); fe_store(oy, i, y); fe_store(ot, i, t); fe_store(oc, i, c);
  valid[i] = (uint8_t)ok;
}

// (ax, ay) = the affine sum ((0, 0) where Z = 0), jz = its Z.  cc: the child chain code the front kernel wrote, zeroed here where the sum is infinite.
__global__ void __launch_bounds__(BLOCK) k_bip32_ckd_pub_accept(const uint64_t* __restrict__ ax, const uint64_t* __restrict__ ay, const uint64_t* __restrict__ jz,
                                                                const uint8_t* __restrict__ valid, uint64_t* __restrict__ cx, uint64_t* __restrict__ cy, uint64_t* cc,
                                                                uint8_t* __restrict__ okv, size_t n) {
  GID;
  const bool ok = valid[i] != 0 && !g_is_zero(fe_load(jz, i));
  fe x = fe_load(ax, i), y = fe_load(ay, i);
  if (!ok) { x = fe_zero(); y = fe_zero(); fe_store(cc, i, x); }
  fe_store(cx, i, x); fe_store(cy, i, y);
  okv[i] = (uint8_t)ok;
}
}  // namespace

namespace launch {
void bip32_master(hipStream_t s, const words8& order, const uint8_t* seed, size_t seed_bytes, size_t stride_bytes, uint64_t* k, uint64_t* c, uint8_t* ok, size_t n) {
  hipLaunchKernelGGL(k_bip32_master, grid_for(n), dim3(BLOCK), 0, s, order, seed, (uint32_t)seed_bytes, stride_bytes, k, c, ok, n);
}
void bip32_ckd_priv(hipStream_t s, const gmod& M, const uint64_t* k_par, const uint64_t* c_par, const uint32_t* index, uint32_t index_all, const uint64_t* xP, const uint64_t* yP,
                    uint64_t* k_child, uint64_t* c_child, uint8_t* ok, size_t n) {
  if (xP) hipLaunchKernelGGL(k_bip32_ckd_priv<true>, grid_for(n), dim3(BLOCK), 0, s, M, k_par, c_par, index, index_all, xP, yP, k_child, c_child, ok, n);
  else hipLaunchKernelGGL(k_bip32_ckd_priv<false>, grid_for(n), dim3(BLOCK), 0, s, M, k_par, c_par, index, index_all, xP, yP, k_child, c_child, ok, n);
}
void bip32_ckd_pub_front(hipStream_t s, const words8& order, const uint64_t* qx, const uint64_t* qy, const uint64_t* c_par, const uint32_t* index, uint32_t index_all, uint64_t* x,
                         uint64_t* y, uint64_t* t, uint64_t* c_child, uint8_t* valid, size_t n) {
  hipLaunchKernelGGL(k_bip32_ckd_pub_front, grid_for(n), dim3(BLOCK), 0, s, order, qx, qy, c_par, index, index_all, x, y, t, c_child, valid, n);
}
void bip32_ckd_pub_accept(hipStream_t s, const uint64_t* ax, const uint64_t* ay, const uint64_t* jz, const uint8_t* valid, uint64_t* cx, uint64_t* cy, uint64_t* c_child, uint8_t* ok,
                          size_t n) {
  hipLaunchKernelGGL(k_bip32_ckd_pub_accept, grid_for(n), dim3(BLOCK), 0, s, ax, ay, jz, valid, cx, cy, c_child, ok, n);
}
}  // namespace launch
}  // namespace ecsimd_hip
