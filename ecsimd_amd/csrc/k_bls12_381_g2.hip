// k_bls12_381_g2.hip -- BLS12-381 G2: the kernels behind ecsimd_bls381_g2_* (include/ecsimd_bls12_381_g2.h).  fp2.cuh is the quadratic extension on fe381.cuh,
// g2.cuh the Jacobian group law with its branches, the scalar product, the subgroup test and the serialisation's rules; msm_stages.cuh has the bucket method's
// stages, which get the group policy g2_group here.  PUBLIC data only: validity, exceptional cases and scalar bits are branches, bucket addresses are scalar digits.
// One lane per element; encodings are big-endian bytes at any alignment (word accesses where an array's base is a multiple of 4: one flag per array).
//
// OUT OF LINE: g2_dbl, g2_add and g2_madd are compiled ONCE in this unit (G2_OP below: noinline) and every kernel calls them.  The G1 unit inlines everything,
// and its k_g1_chunks alone is 117 445 VALU instructions; at three Fp products per Fp2 product the same policy would make this unit several times the size of
// every other unit together, for nothing: a call moves two 72-word points through private memory around roughly 48 Fp products of work.  Everything below the
// three operations (fp2.cuh, fe381.cuh) stays inlined into them.  DESIGN.md 4n has the listing's numbers.
//
// Per lane:  k_g2_decompress, k_g2_compress, k_g2_check, k_g2_mul, k_bls381_g2_raw.
// The sum:   k_g2_digits, k_g2_slices, k_g2_combine, k_g2_chunks, k_g2_tree, k_g2_final (Horner, ONE inversion, the 192-byte result, the flag, the invalid count
//            and the internal check's poisoning as k_g1_final has them); k_g2_tree_affine for the point sum (either encoding), k_g2_products for the LANES route.
// Workspace arrays: an Fp2 element is 96 bytes (c0, then c1, 48 bytes each), element e of an array at byte 96 e; a Jacobian array of `total` elements is three
// such arrays one behind the other (X at e, Y at total + e, Z at 2 total + e).
#include "kernels.h"
#define G2_OP __host__ __device__ __attribute__((noinline)) static
#include "g2.cuh"
#include "bls381_bytes.cuh"
#include "msm_stages.cuh"

namespace ecsimd_hip {
namespace {
using launch::BLOCK;
#define GID size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x; if (i >= n) return

// ---- bytes: records in WIRE order, c1 before c0
ECS_DEV int point192_load(const uint8_t* __restrict__ pts, size_t i, uint32_t aligned, g2_affine& a) {
  const uint8_t* p = pts + 192 * i;
  return g2_decode192(be48_load(p, aligned), be48_load(p + 48, aligned), be48_load(p + 96, aligned), be48_load(p + 144, aligned), a);
}
ECS_DEV int point96_load(const uint8_t* __restrict__ pts, size_t i, uint32_t aligned, g2_affine& a) {
  return g2_decode96(be48_load(pts + 96 * i, aligned), be48_load(pts + 96 * i + 48, aligned), a);
}
ECS_DEV void fill(uint8_t* __restrict__ p, int records, const fe381& v, uint32_t aligned) {
#pragma unroll
  for (int j = 0; j < records; ++j) be48_store(p + 48 * j, v, aligned);
}
ECS_DEV void point192_store(uint8_t* __restrict__ out, size_t i, uint32_t aligned, int cls, const g2_affine& a) {
  fe381 x1w, x0w, y1w, y0w;
  g2_encode192(cls, a, x1w, x0w, y1w, y0w);
  uint8_t* p = out + 192 * i;
  be48_store(p, x1w, aligned); be48_store(p + 48, x0w, aligned); be48_store(p + 96, y1w, aligned); be48_store(p + 144, y0w, aligned);
}
ECS_DEV void point96_store(uint8_t* __restrict__ out, size_t i, uint32_t aligned, int cls, const g2_affine& a) {
  fe381 c1w, c0w;
  g2_encode96(cls, a, c1w, c0w);
  be48_store(out + 96 * i, c1w, aligned); be48_store(out + 96 * i + 48, c0w, aligned);
}
// the encoding of a Jacobian result: one inversion where it is finite
ECS_DEV void jacobian192_store(uint8_t* __restrict__ out, size_t i, uint32_t aligned, const g2_point& P) {
  if (g2_is_identity(P)) point192_store(out, i, aligned, G2_INFINITY, {fp2_zero(), fp2_zero()});
  else point192_store(out, i, aligned, G2_POINT, g2_to_affine(P));
}

// ---- workspace arrays of Fp2 elements
ECS_DEV fp2 ws2_load(const uint64_t* __restrict__ a, size_t e) { return {ws_load(a, 2 * e), ws_load(a, 2 * e + 1)}; }
ECS_DEV void ws2_store(uint64_t* __restrict__ a, size_t e, const fp2& v) { ws_store(a, 2 * e, v.c0); ws_store(a, 2 * e + 1, v.c1); }

// msm_stages.cuh's group: Jacobian accumulators, the terms the affine Montgomery-form points k_g2_digits left at (px, py)
struct g2_group {
  using point = g2_point;
  struct terms { const uint64_t* __restrict__ px; const uint64_t* __restrict__ py; };
  ECS_DEV static point identity() { return g2_identity(); }
  ECS_DEV static point add(const point& P, const point& Q) { return g2_add(P, Q); }
  ECS_DEV static point dbl(const point& P) { return g2_dbl(P); }
  ECS_DEV static point add_term(const point& P, const terms& t, size_t, size_t idx) { return g2_madd(P, {ws2_load(t.px, idx), ws2_load(t.py, idx)}); }
  ECS_DEV static point load(const uint64_t* __restrict__ a, size_t total, size_t e) {
    point R; R.x = ws2_load(a, e); R.y = ws2_load(a, total + e); R.z = ws2_load(a, 2 * total + e); return R;
  }
  ECS_DEV static void store(uint64_t* __restrict__ a, size_t total, size_t e, const point& P) { ws2_store(a, e, P.x); ws2_store(a, total + e, P.y); ws2_store(a, 2 * total + e, P.z); }
};
using G = g2_group;

// ---- per lane
__global__ void __launch_bounds__(BLOCK) k_g2_decompress(const uint8_t* __restrict__ in, uint32_t in_aligned, uint8_t* __restrict__ out, uint32_t out_aligned, uint8_t* __restrict__ ok,
                                                         size_t n) {
  GID;
  g2_affine a;
  const int cls = point96_load(in, i, in_aligned, a);
  if (cls == G2_MALFORMED) fill(out + 192 * i, 4, fe381_zero(), out_aligned);
  else point192_store(out, i, out_aligned, cls, a);
  ok[i] = cls == G2_MALFORMED ? 0 : 1;
}
__global__ void __launch_bounds__(BLOCK) k_g2_compress(const uint8_t* __restrict__ in, uint32_t in_aligned, uint8_t* __restrict__ out, uint32_t out_aligned, uint8_t* __restrict__ ok,
                                                       size_t n) {
  GID;
  g2_affine a;
  const int cls = point192_load(in, i, in_aligned, a);
  if (cls == G2_MALFORMED) fill(out + 96 * i, 2, fe381_zero(), out_aligned);
  else point96_store(out, i, out_aligned, cls, a);
  ok[i] = cls == G2_MALFORMED ? 0 : 1;
}
__global__ void __launch_bounds__(BLOCK) k_g2_check(const uint8_t* __restrict__ in, uint32_t in_aligned, uint8_t* __restrict__ on_curve, uint8_t* __restrict__ in_subgroup, size_t n) {
  GID;
  g2_affine a;
  const int cls = point192_load(in, i, in_aligned, a);
  on_curve[i] = cls == G2_MALFORMED ? 0 : 1;
  in_subgroup[i] = (cls == G2_INFINITY || (cls == G2_POINT && g2_in_subgroup(a))) ? 1 : 0;
}
__global__ void __launch_bounds__(BLOCK) k_g2_mul(const uint64_t* __restrict__ k, const uint8_t* __restrict__ in, uint32_t in_aligned, uint8_t* __restrict__ out, uint32_t out_aligned,
                                                  uint8_t* __restrict__ ok, size_t n) {
  GID;
  g2_affine a;
  const int cls = point192_load(in, i, in_aligned, a);
  if (cls == G2_MALFORMED) { fill(out + 192 * i, 4, fe381_zero(), out_aligned); ok[i] = 0; return; }
  const fe kv = fe_load(k, i);
  jacobian192_store(out, i, out_aligned, cls == G2_POINT ? g2_mul(kv.w, a) : g2_identity());
  ok[i] = 1;
}
// one function of the layers on raw 48-byte records (launch::bls381_g2_raw_inputs / _outputs of them per lane; an Fp2 operand is two records, c0 then c1); every
// 384-bit value is the residue it represents
ECS_DEV void raw2_store(uint8_t* __restrict__ p, const fp2& v, uint32_t aligned) { be48_store(p, fe381_from_mont(v.c0), aligned); be48_store(p + 48, fe381_from_mont(v.c1), aligned); }
__global__ void __launch_bounds__(BLOCK) k_bls381_g2_raw(int op, const uint8_t* __restrict__ in, uint8_t* __restrict__ out, uint32_t aligned, size_t n) {
  GID;
  const int ni = launch::bls381_g2_raw_inputs(op), no = launch::bls381_g2_raw_outputs(op);
  const uint8_t* ip = in + (size_t)48 * ni * i;
  uint8_t* op_ = out + (size_t)48 * no * i;
  const auto rec = [&](int j) { return j < ni ? fe381_to_mont(be48_load(ip + 48 * j, aligned)) : fe381_zero(); };
  const fp2 a = {rec(0), rec(1)}, b = {rec(2), rec(3)};
  if (op < launch::BLS381_G2_RAW_POINT_ADD) {
    fp2 r = a;
    switch (op) {
      case launch::BLS381_G2_RAW_FE2_MUL: r = fp2_mul(a, b); break;
      case launch::BLS381_G2_RAW_FE2_SQR: r = fp2_sqr(a); break;
      case launch::BLS381_G2_RAW_FE2_ADD: r = fp2_add(a, b); break;
      case launch::BLS381_G2_RAW_FE2_SUB: r = fp2_sub(a, b); break;
      case launch::BLS381_G2_RAW_FE2_NEG: r = fp2_neg(a); break;
      case launch::BLS381_G2_RAW_FE2_INVERT: r = fp2_invert(a); break;
      case launch::BLS381_G2_RAW_FE2_SQRT: {
        bool ok;
        r = fp2_sqrt(a, ok);
        be48_store(op_ + 96, fe384_small(ok ? 1u : 0u), aligned);
        break; }
      default: break;                                                   // FE2_CANON
    }
    raw2_store(op_, r, aligned);
    return;
  }
  // x1 = a, y1 = b, id1 = record 4; the second operand from record 5 on
  const g2_point p1 = (fe381_from_mont(rec(4)).w[0] & 1u) ? g2_identity() : g2_from_affine({a, b});
  const g2_affine q2 = {{rec(5), rec(6)}, {rec(7), rec(8)}};
  g2_point R;
  if (op == launch::BLS381_G2_RAW_POINT_ADD) R = g2_add(p1, (fe381_from_mont(rec(9)).w[0] & 1u) ? g2_identity() : g2_from_affine(q2));
  else if (op == launch::BLS381_G2_RAW_POINT_DBL) R = g2_dbl(p1);
  else R = g2_madd(p1, q2);
  const bool id = g2_is_identity(R);
  g2_affine q = {fp2_zero(), fp2_zero()};
  if (!id) q = g2_to_affine(R);
  raw2_store(op_, q.x, aligned); raw2_store(op_ + 96, q.y, aligned);
  be48_store(op_ + 192, fe384_small(id ? 1u : 0u), aligned);
}

// ---- the sum's units
__global__ void __launch_bounds__(BLOCK) k_g2_digits(const uint64_t* __restrict__ k, const uint8_t* __restrict__ pts, uint32_t aligned, uint64_t* __restrict__ kk,
                                                     uint64_t* __restrict__ px, uint64_t* __restrict__ py, uint32_t* __restrict__ hist, uint32_t* __restrict__ counter, size_t n,
                                                     int bits, int c, int windows) {
  GID;
  g2_affine a;
  const int cls = point192_load(pts, i, aligned, a);
  if (cls == G2_MALFORMED) atomicAdd(counter, 1u);
  const fe kv = cls == G2_POINT ? mask_bits(fe_load(k, i), bits) : fe_zero8();
  fe_store(kk, i, kv); ws2_store(px, i, a.x); ws2_store(py, i, a.y);
  msm_histogram(kv, hist, c, windows);
}
__global__ void __launch_bounds__(BLOCK) k_g2_slices(const uint32_t* __restrict__ sorted, const uint64_t* __restrict__ kk, const uint64_t* __restrict__ px,
                                                     const uint64_t* __restrict__ py, const uint32_t* __restrict__ start, uint64_t* __restrict__ buckets,
                                                     uint64_t* __restrict__ partial, uint32_t* __restrict__ broken, size_t n, size_t T, size_t L, size_t slices, int c, size_t K) {
  msm_slices<G>(sorted, kk, {px, py}, start, buckets, partial, broken, n, T, L, slices, c, K);
}
__global__ void __launch_bounds__(BLOCK) k_g2_combine(const uint32_t* __restrict__ start, uint64_t* __restrict__ buckets, const uint64_t* __restrict__ partial,
                                                      uint32_t* __restrict__ broken, size_t L, size_t slices, int c, size_t K) {
  msm_combine<G>(start, buckets, partial, broken, L, slices, c, K);
}
__global__ void __launch_bounds__(BLOCK) k_g2_chunks(const uint64_t* __restrict__ buckets, uint64_t* __restrict__ out, size_t lanes, size_t per_window, int c, int m, size_t K) {
  msm_chunks<G>(buckets, out, lanes, per_window, c, m, K);
}
__global__ void __launch_bounds__(BLOCK) k_g2_tree(uint64_t* arr, size_t total, size_t count, size_t stride, size_t lanes, int fan) {
  msm_tree<G>(arr, total, count, stride, lanes, fan);
}
template <bool COMPRESSED>
__global__ void __launch_bounds__(BLOCK) k_g2_tree_affine(const uint8_t* __restrict__ pts, uint32_t aligned, uint32_t* __restrict__ counter, uint64_t* __restrict__ out, size_t n,
                                                          size_t lanes, int fan) {
  const size_t g = (size_t)blockIdx.x * BLOCK + threadIdx.x;
  if (g >= lanes) return;
  g2_point acc = g2_identity();
#pragma unroll 1
  for (int t = 0; t < fan; ++t) {
    const size_t e = g + (size_t)t * lanes;
    if (e >= n) break;
    g2_affine a;
    const int cls = COMPRESSED ? point96_load(pts, e, aligned, a) : point192_load(pts, e, aligned, a);
    if (cls == G2_MALFORMED) atomicAdd(counter, 1u);
    if (cls != G2_POINT) continue;
    acc = g2_madd(acc, a);
  }
  G::store(out, lanes, g, acc);
}
__global__ void __launch_bounds__(BLOCK) k_g2_products(const uint64_t* __restrict__ k, const uint8_t* __restrict__ pts, uint32_t aligned, uint32_t* __restrict__ counter,
                                                       uint64_t* __restrict__ out, size_t n, int bits) {
  GID;
  g2_affine a;
  const int cls = point192_load(pts, i, aligned, a);
  if (cls == G2_MALFORMED) atomicAdd(counter, 1u);
  const fe kv = mask_bits(fe_load(k, i), bits);
  G::store(out, n, i, cls == G2_POINT ? g2_mul(kv.w, a) : g2_identity());
}
// One lane: msm_horner, then the 192-byte result.
__global__ void __launch_bounds__(64) k_g2_final(const uint64_t* __restrict__ arr, size_t total, size_t stride, int windows, int c, const uint32_t* __restrict__ counter,
                                                 uint8_t* __restrict__ out, uint32_t aligned, uint8_t* __restrict__ finite, uint32_t* __restrict__ invalid) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const g2_point acc = msm_horner<G>(arr, total, stride, windows, c);
  const bool fin = !g2_is_identity(acc);
  uint32_t bad = counter ? counter[0] : 0u;
  if (counter && counter[1] != 0u) {                                    // a broken invariant of the sort: no sum is better than a wrong one (ecsimd_msm.h, INTERNAL CHECK)
    fe381 ones;
#pragma unroll
    for (int j = 0; j < 12; ++j) ones.w[j] = 0xffffffffu;
    fill(out, 4, ones, aligned);
    bad = 0xffffffffu;
  } else jacobian192_store(out, 0, aligned, acc);
  finite[0] = (uint8_t)((fin || bad == 0xffffffffu) ? 1 : 0);
  if (invalid) invalid[0] = bad;
}
}  // namespace

namespace launch {
static uint32_t word_aligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0 ? 1u : 0u; }
static dim3 grid_of(size_t lanes, size_t y = 1) { return dim3((unsigned)((lanes + BLOCK - 1) / BLOCK), (unsigned)y); }
void bls381_g2_decompress(hipStream_t s, const uint8_t* in96, uint8_t* out192, uint8_t* ok, size_t n) {
  hipLaunchKernelGGL(k_g2_decompress, grid_for(n), dim3(BLOCK), 0, s, in96, word_aligned(in96), out192, word_aligned(out192), ok, n);
}
void bls381_g2_compress(hipStream_t s, const uint8_t* in192, uint8_t* out96, uint8_t* ok, size_t n) {
  hipLaunchKernelGGL(k_g2_compress, grid_for(n), dim3(BLOCK), 0, s, in192, word_aligned(in192), out96, word_aligned(out96), ok, n);
}
void bls381_g2_check(hipStream_t s, const uint8_t* in192, uint8_t* on_curve, uint8_t* in_subgroup, size_t n) {
  hipLaunchKernelGGL(k_g2_check, grid_for(n), dim3(BLOCK), 0, s, in192, word_aligned(in192), on_curve, in_subgroup, n);
}
void bls381_g2_mul(hipStream_t s, const uint64_t* k, const uint8_t* in192, uint8_t* out192, uint8_t* ok, size_t n) {
  hipLaunchKernelGGL(k_g2_mul, grid_for(n), dim3(BLOCK), 0, s, k, in192, word_aligned(in192), out192, word_aligned(out192), ok, n);
}
void bls381_g2_raw(hipStream_t s, int op, const uint8_t* in, uint8_t* out, size_t n) {
  hipLaunchKernelGGL(k_bls381_g2_raw, grid_for(n), dim3(BLOCK), 0, s, op, in, out, word_aligned(in) & word_aligned(out), n);
}
void g2_msm_launch::digits(hipStream_t s, const uint64_t* k, const uint8_t* pts192, uint64_t* kk, uint64_t* px, uint64_t* py, uint32_t* hist, uint32_t* counter, size_t n, int bits,
                           int c, int windows) {
  hipLaunchKernelGGL(k_g2_digits, grid_of(n), dim3(BLOCK), 0, s, k, pts192, word_aligned(pts192), kk, px, py, hist, counter, n, bits, c, windows);
}
void g2_msm_launch::slices(hipStream_t s, const uint32_t* sorted, const uint64_t* kk, const uint64_t* px, const uint64_t* py, const uint32_t* start, uint64_t* buckets,
                           uint64_t* partial, uint32_t* broken, size_t n, size_t T, size_t L, size_t slices, int c, size_t K) {
  hipLaunchKernelGGL(k_g2_slices, grid_of(slices), dim3(BLOCK), 0, s, sorted, kk, px, py, start, buckets, partial, broken, n, T, L, slices, c, K);
}
void g2_msm_launch::combine(hipStream_t s, const uint32_t* start, uint64_t* buckets, const uint64_t* partial, uint32_t* broken, size_t L, size_t slices, int c, size_t K) {
  hipLaunchKernelGGL(k_g2_combine, grid_of(K), dim3(BLOCK), 0, s, start, buckets, partial, broken, L, slices, c, K);
}
void g2_msm_launch::chunks(hipStream_t s, const uint64_t* buckets, uint64_t* out, size_t lanes, size_t per_window, int c, int m, size_t K) {
  hipLaunchKernelGGL(k_g2_chunks, grid_of(lanes), dim3(BLOCK), 0, s, buckets, out, lanes, per_window, c, m, K);
}
void g2_msm_launch::tree(hipStream_t s, uint64_t* arr, size_t total, size_t count, size_t stride, size_t groups, size_t lanes, int fan) {
  hipLaunchKernelGGL(k_g2_tree, grid_of(lanes, groups), dim3(BLOCK), 0, s, arr, total, count, stride, lanes, fan);
}
void g2_msm_launch::tree_affine(hipStream_t s, const uint8_t* pts, bool compressed, uint32_t* counter, uint64_t* out, size_t n, size_t lanes, int fan) {
  if (compressed) hipLaunchKernelGGL(k_g2_tree_affine<true>, grid_of(lanes), dim3(BLOCK), 0, s, pts, word_aligned(pts), counter, out, n, lanes, fan);
  else hipLaunchKernelGGL(k_g2_tree_affine<false>, grid_of(lanes), dim3(BLOCK), 0, s, pts, word_aligned(pts), counter, out, n, lanes, fan);
}
void g2_msm_launch::products(hipStream_t s, const uint64_t* k, const uint8_t* pts192, uint32_t* counter, uint64_t* out, size_t n, int bits) {
  hipLaunchKernelGGL(k_g2_products, grid_of(n), dim3(BLOCK), 0, s, k, pts192, word_aligned(pts192), counter, out, n, bits);
}
void g2_msm_launch::finish(hipStream_t s, const uint64_t* arr, size_t total, size_t stride, int windows, int c, const uint32_t* counter, uint8_t* out192, uint8_t* finite,
                           uint32_t* invalid) {
  hipLaunchKernelGGL(k_g2_final, dim3(1), dim3(64), 0, s, arr, total, stride, windows, c, counter, out192, word_aligned(out192), finite, invalid);
}
}  // namespace launch
}  // namespace ecsimd_hip
