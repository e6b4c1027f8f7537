// k_bls12_381.hip -- BLS12-381 G1: the kernels behind ecsimd_bls12_381_g1_* and ecsimd_bls12_381_raw (include/ecsimd_bls12_381.h).  fe381.cuh is the field
// (Montgomery form, canonical), g1.cuh the Jacobian group law with its branches, the scalar product, the subgroup test and the serialisation's rules;
// msm_stages.cuh has the bucket method's stages, which get the group policy g1_group here.  PUBLIC data only: validity, exceptional cases and scalar bits are
// branches, bucket addresses are scalar digits.  One lane per element; encodings are big-endian bytes at any alignment (word accesses where an array's base is
// a multiple of 4: one flag per array).
//
// Per lane:  k_g1_decompress, k_g1_compress, k_g1_check, k_g1_mul, k_bls381_raw.
// The sum:   k_g1_digits (decode, validate, Montgomery form, the masked scalar, the histogram), k_g1_slices, k_g1_combine, k_g1_chunks, k_g1_tree, k_g1_final
//            (Horner, ONE inversion, the 96-byte result, the flag, the invalid count and the internal check's poisoning as k_msm_final has them);
//            k_g1_tree_affine for the point sum (either encoding), k_g1_products for the LANES route.
// Workspace arrays: a field element is 48 bytes (three uint4), element e of an array at byte 48 e; a Jacobian array of `total` elements is three such arrays one
// behind the other (X at e, Y at total + e, Z at 2 total + e).
#include "kernels.h"
#include "g1.cuh"
#include "bls381_bytes.cuh"
#include "msm_stages.cuh"

namespace ecsimd_hip {
namespace {
using launch::BLOCK;
#define GID size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x; if (i >= n) return

// ---- bytes (be48_load / be48_store: bls381_bytes.cuh)
// record i of an array of 96-byte (48-byte) encodings, decoded: G1_INFINITY, G1_POINT (a in Montgomery form) or G1_MALFORMED
ECS_DEV int point96_load(const uint8_t* __restrict__ pts, size_t i, uint32_t aligned, g1_affine& a) {
  return g1_decode96(be48_load(pts + 96 * i, aligned), be48_load(pts + 96 * i + 48, aligned), a);
}
ECS_DEV int point48_load(const uint8_t* __restrict__ pts, size_t i, uint32_t aligned, g1_affine& a) { return g1_decode48(be48_load(pts + 48 * i, aligned), a); }
ECS_DEV void point96_store(uint8_t* __restrict__ out, size_t i, uint32_t aligned, int cls, const g1_affine& a) {
  fe381 xw, yw;
  g1_encode96(cls, a, xw, yw);
  be48_store(out + 96 * i, xw, aligned); be48_store(out + 96 * i + 48, yw, aligned);
}
// the encoding of a Jacobian result: one inversion where it is finite
ECS_DEV void jacobian96_store(uint8_t* __restrict__ out, size_t i, uint32_t aligned, const g1_point& P) {
  if (g1_is_identity(P)) point96_store(out, i, aligned, G1_INFINITY, {fe381_zero(), fe381_zero()});
  else point96_store(out, i, aligned, G1_POINT, g1_to_affine(P));
}

// ---- workspace arrays: ws_load / ws_store / fe_zero8 are bls381_bytes.cuh's, shared with the G2 unit

// msm_stages.cuh's group: Jacobian accumulators, the terms the affine Montgomery-form points k_g1_digits left at (px, py)
struct g1_group {
  using point = g1_point;
  struct terms { const uint64_t* __restrict__ px; const uint64_t* __restrict__ py; };
  ECS_DEV static point identity() { return g1_identity(); }
  ECS_DEV static point add(const point& P, const point& Q) { return g1_add(P, Q); }
  ECS_DEV static point dbl(const point& P) { return g1_dbl(P); }
  ECS_DEV static point add_term(const point& P, const terms& t, size_t, size_t idx) { return g1_madd(P, ws_load(t.px, idx), ws_load(t.py, idx)); }
  ECS_DEV static point load(const uint64_t* __restrict__ a, size_t total, size_t e) {
    point R; R.x = ws_load(a, e); R.y = ws_load(a, total + e); R.z = ws_load(a, 2 * total + e); return R;
  }
  ECS_DEV static void store(uint64_t* __restrict__ a, size_t total, size_t e, const point& P) { ws_store(a, e, P.x); ws_store(a, total + e, P.y); ws_store(a, 2 * total + e, P.z); }
};
using G = g1_group;

// ---- per lane
__global__ void __launch_bounds__(BLOCK) k_g1_decompress(const uint8_t* __restrict__ in, uint32_t in_aligned, uint8_t* __restrict__ out, uint32_t out_aligned, uint8_t* __restrict__ ok,
                                                         size_t n) {
  GID;
  g1_affine a;
  const int cls = point48_load(in, i, in_aligned, a);
  if (cls == G1_MALFORMED) { be48_store(out + 96 * i, fe381_zero(), out_aligned); be48_store(out + 96 * i + 48, fe381_zero(), out_aligned); }
  else point96_store(out, i, out_aligned, cls, a);
  ok[i] = cls == G1_MALFORMED ? 0 : 1;
}
__global__ void __launch_bounds__(BLOCK) k_g1_compress(const uint8_t* __restrict__ in, uint32_t in_aligned, uint8_t* __restrict__ out, uint32_t out_aligned, uint8_t* __restrict__ ok,
                                                       size_t n) {
  GID;
  g1_affine a;
  const int cls = point96_load(in, i, in_aligned, a);
  be48_store(out + 48 * i, cls == G1_MALFORMED ? fe381_zero() : g1_encode48(cls, a), out_aligned);
  ok[i] = cls == G1_MALFORMED ? 0 : 1;
}
__global__ void __launch_bounds__(BLOCK) k_g1_check(const uint8_t* __restrict__ in, uint32_t in_aligned, uint8_t* __restrict__ on_curve, uint8_t* __restrict__ in_subgroup, size_t n) {
  GID;
  g1_affine a;
  const int cls = point96_load(in, i, in_aligned, a);
  on_curve[i] = cls == G1_MALFORMED ? 0 : 1;
  in_subgroup[i] = (cls == G1_INFINITY || (cls == G1_POINT && g1_in_subgroup(a))) ? 1 : 0;
}
__global__ void __launch_bounds__(BLOCK) k_g1_mul(const uint64_t* __restrict__ k, const uint8_t* __restrict__ in, uint32_t in_aligned, uint8_t* __restrict__ out, uint32_t out_aligned,
                                                  uint8_t* __restrict__ ok, size_t n) {
  GID;
  g1_affine a;
  const int cls = point96_load(in, i, in_aligned, a);
  if (cls == G1_MALFORMED) { be48_store(out + 96 * i, fe381_zero(), out_aligned); be48_store(out + 96 * i + 48, fe381_zero(), out_aligned); ok[i] = 0; return; }
  const fe kv = fe_load(k, i);
  jacobian96_store(out, i, out_aligned, cls == G1_POINT ? g1_mul(kv.w, a) : g1_identity());
  ok[i] = 1;
}
// one function of the layers on raw 48-byte records (launch::bls381_raw_inputs / _outputs of them per lane); every 384-bit value is the residue it represents
__global__ void __launch_bounds__(BLOCK) k_bls381_raw(int op, const uint8_t* __restrict__ in, uint8_t* __restrict__ out, uint32_t aligned, size_t n) {
  GID;
  const int ni = launch::bls381_raw_inputs(op), no = launch::bls381_raw_outputs(op);
  const uint8_t* ip = in + (size_t)48 * ni * i;
  uint8_t* op_ = out + (size_t)48 * no * i;
  fe381 a[6];
#pragma unroll
  for (int j = 0; j < 6; ++j) a[j] = j < ni ? fe381_to_mont(be48_load(ip + 48 * j, aligned)) : fe381_zero();
  if (op < launch::BLS381_RAW_POINT_ADD) {
    fe381 r = a[0];
    switch (op) {
      case launch::BLS381_RAW_FE_MUL: r = fe381_mul(a[0], a[1]); break;
      case launch::BLS381_RAW_FE_SQR: r = fe381_sqr(a[0]); break;
      case launch::BLS381_RAW_FE_ADD: r = fe381_add(a[0], a[1]); break;
      case launch::BLS381_RAW_FE_SUB: r = fe381_sub(a[0], a[1]); break;
      case launch::BLS381_RAW_FE_NEG: r = fe381_neg(a[0]); break;
      case launch::BLS381_RAW_FE_INVERT: r = fe381_invert(a[0]); break;
      case launch::BLS381_RAW_FE_SQRT: {
        bool ok;
        r = fe381_sqrt(a[0], ok);
        be48_store(op_ + 48, fe384_small(ok ? 1u : 0u), aligned);
        break; }
      default: break;                                                   // FE_CANON
    }
    be48_store(op_, fe381_from_mont(r), aligned);
    return;
  }
  const g1_point p1 = (fe381_from_mont(a[2]).w[0] & 1u) ? g1_identity() : g1_from_affine({a[0], a[1]});
  g1_point R;
  if (op == launch::BLS381_RAW_POINT_ADD) R = g1_add(p1, (fe381_from_mont(a[5]).w[0] & 1u) ? g1_identity() : g1_from_affine({a[3], a[4]}));
  else if (op == launch::BLS381_RAW_POINT_DBL) R = g1_dbl(p1);
  else R = g1_madd(p1, a[3], a[4]);
  const bool id = g1_is_identity(R);
  g1_affine q = {fe381_zero(), fe381_zero()};
  if (!id) q = g1_to_affine(R);
  be48_store(op_, fe381_from_mont(q.x), aligned);
  be48_store(op_ + 48, fe381_from_mont(q.y), aligned);
  be48_store(op_ + 96, fe384_small(id ? 1u : 0u), aligned);
}

// ---- the sum's units
__global__ void __launch_bounds__(BLOCK) k_g1_digits(const uint64_t* __restrict__ k, const uint8_t* __restrict__ pts, uint32_t aligned, uint64_t* __restrict__ kk,
                                                     uint64_t* __restrict__ px, uint64_t* __restrict__ py, uint32_t* __restrict__ hist, uint32_t* __restrict__ counter, size_t n,
                                                     int bits, int c, int windows) {
  GID;
  g1_affine a;
  const int cls = point96_load(pts, i, aligned, a);
  if (cls == G1_MALFORMED) atomicAdd(counter, 1u);
  const fe kv = cls == G1_POINT ? mask_bits(fe_load(k, i), bits) : fe_zero8();
  fe_store(kk, i, kv); ws_store(px, i, a.x); ws_store(py, i, a.y);
  msm_histogram(kv, hist, c, windows);
}
__global__ void __launch_bounds__(BLOCK) k_g1_slices(const uint32_t* __restrict__ sorted, const uint64_t* __restrict__ kk, const uint64_t* __restrict__ px,
                                                     const uint64_t* __restrict__ py, const uint32_t* __restrict__ start, uint64_t* __restrict__ buckets,
                                                     uint64_t* __restrict__ partial, uint32_t* __restrict__ broken, size_t n, size_t T, size_t L, size_t slices, int c, size_t K) {
  msm_slices<G>(sorted, kk, {px, py}, start, buckets, partial, broken, n, T, L, slices, c, K);
}
__global__ void __launch_bounds__(BLOCK) k_g1_combine(const uint32_t* __restrict__ start, uint64_t* __restrict__ buckets, const uint64_t* __restrict__ partial,
                                                      uint32_t* __restrict__ broken, size_t L, size_t slices, int c, size_t K) {
  msm_combine<G>(start, buckets, partial, broken, L, slices, c, K);
}
__global__ void __launch_bounds__(BLOCK) k_g1_chunks(const uint64_t* __restrict__ buckets, uint64_t* __restrict__ out, size_t lanes, size_t per_window, int c, int m, size_t K) {
  msm_chunks<G>(buckets, out, lanes, per_window, c, m, K);
}
__global__ void __launch_bounds__(BLOCK) k_g1_tree(uint64_t* arr, size_t total, size_t count, size_t stride, size_t lanes, int fan) {
  msm_tree<G>(arr, total, count, stride, lanes, fan);
}
template <bool COMPRESSED>
__global__ void __launch_bounds__(BLOCK) k_g1_tree_affine(const uint8_t* __restrict__ pts, uint32_t aligned, uint32_t* __restrict__ counter, uint64_t* __restrict__ out, size_t n,
                                                          size_t lanes, int fan) {
  const size_t g = (size_t)blockIdx.x * BLOCK + threadIdx.x;
  if (g >= lanes) return;
  g1_point acc = g1_identity();
#pragma unroll 1
  for (int t = 0; t < fan; ++t) {
    const size_t e = g + (size_t)t * lanes;
    if (e >= n) break;
    g1_affine a;
    const int cls = COMPRESSED ? point48_load(pts, e, aligned, a) : point96_load(pts, e, aligned, a);
    if (cls == G1_MALFORMED) atomicAdd(counter, 1u);
    if (cls != G1_POINT) continue;
    acc = g1_madd(acc, a.x, a.y);
  }
  G::store(out, lanes, g, acc);
}
__global__ void __launch_bounds__(BLOCK) k_g1_products(const uint64_t* __restrict__ k, const uint8_t* __restrict__ pts, uint32_t aligned, uint32_t* __restrict__ counter,
                                                       uint64_t* __restrict__ out, size_t n, int bits) {
  GID;
  g1_affine a;
  const int cls = point96_load(pts, i, aligned, a);
  if (cls == G1_MALFORMED) atomicAdd(counter, 1u);
  const fe kv = mask_bits(fe_load(k, i), bits);
  G::store(out, n, i, cls == G1_POINT ? g1_mul(kv.w, a) : g1_identity());
}
// One lane: msm_horner, then the 96-byte result.
__global__ void __launch_bounds__(64) k_g1_final(const uint64_t* __restrict__ arr, size_t total, size_t stride, int windows, int c, const uint32_t* __restrict__ counter,
                                                 uint8_t* __restrict__ out, uint32_t aligned, uint8_t* __restrict__ finite, uint32_t* __restrict__ invalid) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const g1_point acc = msm_horner<G>(arr, total, stride, windows, c);
  const bool fin = !g1_is_identity(acc);
  uint32_t bad = counter ? counter[0] : 0u;
  if (counter && counter[1] != 0u) {                                    // a broken invariant of the sort: no sum is better than a wrong one (ecsimd_msm.h, INTERNAL CHECK)
    fe381 ones;
#pragma unroll
    for (int j = 0; j < 12; ++j) ones.w[j] = 0xffffffffu;
    be48_store(out, ones, aligned); be48_store(out + 48, ones, aligned);
    bad = 0xffffffffu;
  } else jacobian96_store(out, 0, aligned, acc);
  finite[0] = (uint8_t)((fin || bad == 0xffffffffu) ? 1 : 0);
  if (invalid) invalid[0] = bad;
}
}  // namespace

namespace launch {
static uint32_t word_aligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0 ? 1u : 0u; }
static dim3 grid_of(size_t lanes, size_t y = 1) { return dim3((unsigned)((lanes + BLOCK - 1) / BLOCK), (unsigned)y); }
void bls381_g1_decompress(hipStream_t s, const uint8_t* in48, uint8_t* out96, uint8_t* ok, size_t n) {
  hipLaunchKernelGGL(k_g1_decompress, grid_for(n), dim3(BLOCK), 0, s, in48, word_aligned(in48), out96, word_aligned(out96), ok, n);
}
void bls381_g1_compress(hipStream_t s, const uint8_t* in96, uint8_t* out48, uint8_t* ok, size_t n) {
  hipLaunchKernelGGL(k_g1_compress, grid_for(n), dim3(BLOCK), 0, s, in96, word_aligned(in96), out48, word_aligned(out48), ok, n);
}
void bls381_g1_check(hipStream_t s, const uint8_t* in96, uint8_t* on_curve, uint8_t* in_subgroup, size_t n) {
  hipLaunchKernelGGL(k_g1_check, grid_for(n), dim3(BLOCK), 0, s, in96, word_aligned(in96), on_curve, in_subgroup, n);
}
void bls381_g1_mul(hipStream_t s, const uint64_t* k, const uint8_t* in96, uint8_t* out96, uint8_t* ok, size_t n) {
  hipLaunchKernelGGL(k_g1_mul, grid_for(n), dim3(BLOCK), 0, s, k, in96, word_aligned(in96), out96, word_aligned(out96), ok, n);
}
void bls381_raw(hipStream_t s, int op, const uint8_t* in, uint8_t* out, size_t n) {
  hipLaunchKernelGGL(k_bls381_raw, grid_for(n), dim3(BLOCK), 0, s, op, in, out, word_aligned(in) & word_aligned(out), n);
}
void g1_msm_launch::digits(hipStream_t s, const uint64_t* k, const uint8_t* pts96, uint64_t* kk, uint64_t* px, uint64_t* py, uint32_t* hist, uint32_t* counter, size_t n, int bits,
                           int c, int windows) {
  hipLaunchKernelGGL(k_g1_digits, grid_of(n), dim3(BLOCK), 0, s, k, pts96, word_aligned(pts96), kk, px, py, hist, counter, n, bits, c, windows);
}
void g1_msm_launch::slices(hipStream_t s, const uint32_t* sorted, const uint64_t* kk, const uint64_t* px, const uint64_t* py, const uint32_t* start, uint64_t* buckets,
                           uint64_t* partial, uint32_t* broken, size_t n, size_t T, size_t L, size_t slices, int c, size_t K) {
  hipLaunchKernelGGL(k_g1_slices, grid_of(slices), dim3(BLOCK), 0, s, sorted, kk, px, py, start, buckets, partial, broken, n, T, L, slices, c, K);
}
void g1_msm_launch::combine(hipStream_t s, const uint32_t* start, uint64_t* buckets, const uint64_t* partial, uint32_t* broken, size_t L, size_t slices, int c, size_t K) {
  hipLaunchKernelGGL(k_g1_combine, grid_of(K), dim3(BLOCK), 0, s, start, buckets, partial, broken, L, slices, c, K);
}
void g1_msm_launch::chunks(hipStream_t s, const uint64_t* buckets, uint64_t* out, size_t lanes, size_t per_window, int c, int m, size_t K) {
  hipLaunchKernelGGL(k_g1_chunks, grid_of(lanes), dim3(BLOCK), 0, s, buckets, out, lanes, per_window, c, m, K);
}
void g1_msm_launch::tree(hipStream_t s, uint64_t* arr, size_t total, size_t count, size_t stride, size_t groups, size_t lanes, int fan) {
  hipLaunchKernelGGL(k_g1_tree, grid_of(lanes, groups), dim3(BLOCK), 0, s, arr, total, count, stride, lanes, fan);
}
void g1_msm_launch::tree_affine(hipStream_t s, const uint8_t* pts, bool compressed, uint32_t* counter, uint64_t* out, size_t n, size_t lanes, int fan) {
  if (compressed) hipLaunchKernelGGL(k_g1_tree_affine<true>, grid_of(lanes), dim3(BLOCK), 0, s, pts, word_aligned(pts), counter, out, n, lanes, fan);
  else hipLaunchKernelGGL(k_g1_tree_affine<false>, grid_of(lanes), dim3(BLOCK), 0, s, pts, word_aligned(pts), counter, out, n, lanes, fan);
}
void g1_msm_launch::products(hipStream_t s, const uint64_t* k, const uint8_t* pts96, uint32_t* counter, uint64_t* out, size_t n, int bits) {
  hipLaunchKernelGGL(k_g1_products, grid_of(n), dim3(BLOCK), 0, s, k, pts96, word_aligned(pts96), counter, out, n, bits);
}
void g1_msm_launch::finish(hipStream_t s, const uint64_t* arr, size_t total, size_t stride, int windows, int c, const uint32_t* counter, uint8_t* out96, uint8_t* finite,
                           uint32_t* invalid) {
  hipLaunchKernelGGL(k_g1_final, dim3(1), dim3(64), 0, s, arr, total, stride, windows, c, counter, out96, word_aligned(out96), finite, invalid);
}
}  // namespace launch
}  // namespace ecsimd_hip
