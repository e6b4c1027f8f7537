// k_bls12_381.inc -- the kernels of a BLS12-381 group and their launchers, ONCE: k_bls12_381.hip includes this text after g1.cuh (behind ecsimd_bls12_381_g1_* and
// ecsimd_bls12_381_raw), k_bls12_381_g2.hip after g2.cuh (behind ecsimd_bls381_g2_*), each having chosen its inlining policy first (bls381_curve.inc).  It reads the
// group header's policy (BLS381_G, BLS381_F, BLS381_ELEM, BLS381_COMPONENTS, and BLS381_Q2 / BLS381_Q2_OF for a mixed addition's operand) and, from the
// unit, BLS381_K(stage), the kernels' names, BLS381_K_RAW, the unit's own raw kernel (defined before this text: see there why), and BLS381_LAUNCH, the
// instance of launch::bls381_launch it defines.  msm_stages.cuh has the bucket method's stages, which get the group policy
// msm_group here.  PUBLIC data only: validity, exceptional cases and scalar bits are branches, bucket addresses are scalar digits.  One lane per element; encodings
// are big-endian bytes at any alignment (word accesses where an array's base is a multiple of 4: one flag per array).
//
// Per lane:  decompress, compress, check, mul.
// The sum:   digits (decode, validate, Montgomery form, the masked scalar, the histogram), slices, combine, chunks, tree, final (Horner, ONE inversion, the
//            uncompressed result, the flag, the invalid count and the internal check's poisoning as k_msm_final has them); tree_affine for the point sum (either
//            encoding), products for the LANES route.
// With NC = BLS381_COMPONENTS: an encoding is 2 NC (compressed: NC) 48-byte records in wire order; a field element in the workspace is NC fe381 elements of
// bls381_bytes.cuh, least significant component first, element e of an array at byte 48 NC e; a Jacobian array of `total` elements is three such arrays one behind
// the other (X at e, Y at total + e, Z at 2 total + e).
#include "kernels.h"
#include "bls381_bytes.cuh"
#include "msm_stages.cuh"

#define G_ BLS381_G
#define F_ BLS381_F
#define FE BLS381_ELEM
#define NC BLS381_COMPONENTS
#define K_ BLS381_K

namespace ecsimd_hip {
namespace {
using launch::BLOCK;
#define GID size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x; if (i >= n) return

// ---- bytes (be48_load / be48_store: bls381_bytes.cuh)
template <int N> ECS_DEV void records_load(const uint8_t* __restrict__ p, uint32_t aligned, fe381 (&w)[N]) {
#pragma unroll
  for (int j = 0; j < N; ++j) w[j] = be48_load(p + 48 * j, aligned);
}
template <int N> ECS_DEV void records_store(uint8_t* __restrict__ p, uint32_t aligned, const fe381 (&w)[N]) {
#pragma unroll
  for (int j = 0; j < N; ++j) be48_store(p + 48 * j, w[j], aligned);
}
ECS_DEV void fill(uint8_t* __restrict__ p, int records, const fe381& v, uint32_t aligned) {
#pragma unroll
  for (int j = 0; j < records; ++j) be48_store(p + 48 * j, v, aligned);
}
// record i of an array of uncompressed (compressed) encodings, decoded: BLS381_INFINITY, BLS381_POINT (a in Montgomery form) or BLS381_MALFORMED
ECS_DEV int point_load(const uint8_t* __restrict__ pts, size_t i, uint32_t aligned, G_(affine)& a) {
  fe381 w[2 * NC];
  records_load(pts + sizeof w * i, aligned, w);
  return G_(decode)(w, a);
}
ECS_DEV int compressed_load(const uint8_t* __restrict__ pts, size_t i, uint32_t aligned, G_(affine)& a) {
  fe381 w[NC];
  records_load(pts + sizeof w * i, aligned, w);
  return G_(decode_compressed)(w, a);
}
ECS_DEV void point_store(uint8_t* __restrict__ out, size_t i, uint32_t aligned, int cls, const G_(affine)& a) {
  fe381 w[2 * NC];
  G_(encode)(cls, a, w);
  records_store(out + sizeof w * i, aligned, w);
}
// cls may be BLS381_MALFORMED here: zeros
ECS_DEV void compressed_store(uint8_t* __restrict__ out, size_t i, uint32_t aligned, int cls, const G_(affine)& a) {
  fe381 w[NC];
  G_(encode_compressed)(cls, a, w);
  records_store(out + sizeof w * i, aligned, w);
}
// the encoding of a Jacobian result: one inversion where it is finite
ECS_DEV void jacobian_store(uint8_t* __restrict__ out, size_t i, uint32_t aligned, const G_(point)& P) {
  if (G_(is_identity)(P)) point_store(out, i, aligned, BLS381_INFINITY, {F_(zero)(), F_(zero)()});
  else point_store(out, i, aligned, BLS381_POINT, G_(to_affine)(P));
}

// ---- workspace arrays of field elements (ws_load / ws_store / fe_zero8: bls381_bytes.cuh)
ECS_DEV FE elem_load(const uint64_t* __restrict__ a, size_t e) {
  FE v;
#pragma unroll
  for (int t = 0; t < NC; ++t) F_(component)(v, t) = ws_load(a, NC * e + t);
  return v;
}
ECS_DEV void elem_store(uint64_t* __restrict__ a, size_t e, const FE& v) {
#pragma unroll
  for (int t = 0; t < NC; ++t) ws_store(a, NC * e + t, F_(component)(v, t));
}

// msm_stages.cuh's group: Jacobian accumulators, the terms the affine Montgomery-form points the digits kernel left at (px, py)
struct msm_group {
  using point = G_(point);
  struct terms { const uint64_t* __restrict__ px; const uint64_t* __restrict__ py; };
  ECS_DEV static point identity() { return G_(identity)(); }
  ECS_DEV static point add(const point& P, const point& Q) { return G_(add)(P, Q); }
  ECS_DEV static point dbl(const point& P) { return G_(dbl)(P); }
  ECS_DEV static point add_term(const point& P, const terms& t, size_t, size_t idx) { return G_(madd)(P, BLS381_Q2_OF(elem_load(t.px, idx), elem_load(t.py, idx))); }
  ECS_DEV static point load(const uint64_t* __restrict__ a, size_t total, size_t e) {
    point R; R.x = elem_load(a, e); R.y = elem_load(a, total + e); R.z = elem_load(a, 2 * total + e); return R;
  }
  ECS_DEV static void store(uint64_t* __restrict__ a, size_t total, size_t e, const point& P) { elem_store(a, e, P.x); elem_store(a, total + e, P.y); elem_store(a, 2 * total + e, P.z); }
};
using G = msm_group;

// ---- per lane
__global__ void __launch_bounds__(BLOCK) K_(decompress)(const uint8_t* __restrict__ in, uint32_t in_aligned, uint8_t* __restrict__ out, uint32_t out_aligned, uint8_t* __restrict__ ok,
                                                        size_t n) {
  GID;
  G_(affine) a;
  const int cls = compressed_load(in, i, in_aligned, a);
  if (cls == BLS381_MALFORMED) fill(out + 96 * NC * i, 2 * NC, fe381_zero(), out_aligned);
  else point_store(out, i, out_aligned, cls, a);
  ok[i] = cls == BLS381_MALFORMED ? 0 : 1;
}
__global__ void __launch_bounds__(BLOCK) K_(compress)(const uint8_t* __restrict__ in, uint32_t in_aligned, uint8_t* __restrict__ out, uint32_t out_aligned, uint8_t* __restrict__ ok,
                                                      size_t n) {
  GID;
  G_(affine) a;
  const int cls = point_load(in, i, in_aligned, a);
  compressed_store(out, i, out_aligned, cls, a);
  ok[i] = cls == BLS381_MALFORMED ? 0 : 1;
}
__global__ void __launch_bounds__(BLOCK) K_(check)(const uint8_t* __restrict__ in, uint32_t in_aligned, uint8_t* __restrict__ on_curve, uint8_t* __restrict__ in_subgroup, size_t n) {
  GID;
  G_(affine) a;
  const int cls = point_load(in, i, in_aligned, a);
  on_curve[i] = cls == BLS381_MALFORMED ? 0 : 1;
  in_subgroup[i] = (cls == BLS381_INFINITY || (cls == BLS381_POINT && G_(in_subgroup)(a))) ? 1 : 0;
}
__global__ void __launch_bounds__(BLOCK) K_(mul)(const uint64_t* __restrict__ k, const uint8_t* __restrict__ in, uint32_t in_aligned, uint8_t* __restrict__ out, uint32_t out_aligned,
                                                 uint8_t* __restrict__ ok, size_t n) {
  GID;
  G_(affine) a;
  const int cls = point_load(in, i, in_aligned, a);
  if (cls == BLS381_MALFORMED) { fill(out + 96 * NC * i, 2 * NC, fe381_zero(), out_aligned); ok[i] = 0; return; }
  const fe kv = fe_load(k, i);
  jacobian_store(out, i, out_aligned, cls == BLS381_POINT ? G_(mul)(kv.w, a) : G_(identity)());
  ok[i] = 1;
}
// ---- the sum's units
__global__ void __launch_bounds__(BLOCK) K_(digits)(const uint64_t* __restrict__ k, const uint8_t* __restrict__ pts, uint32_t aligned, uint64_t* __restrict__ kk,
                                                    uint64_t* __restrict__ px, uint64_t* __restrict__ py, uint32_t* __restrict__ hist, uint32_t* __restrict__ counter, size_t n,
                                                    int bits, int c, int windows) {
  GID;
  G_(affine) a;
  const int cls = point_load(pts, i, aligned, a);
  if (cls == BLS381_MALFORMED) atomicAdd(counter, 1u);
  const fe kv = cls == BLS381_POINT ? mask_bits(fe_load(k, i), bits) : fe_zero8();
  fe_store(kk, i, kv); elem_store(px, i, a.x); elem_store(py, i, a.y);
  msm_histogram(kv, hist, c, windows);
}
__global__ void __launch_bounds__(BLOCK) K_(slices)(const uint32_t* __restrict__ sorted, const uint64_t* __restrict__ kk, const uint64_t* __restrict__ px,
                                                    const uint64_t* __restrict__ py, const uint32_t* __restrict__ start, uint64_t* __restrict__ buckets,
                                                    uint64_t* __restrict__ partial, uint32_t* __restrict__ broken, size_t n, size_t T, size_t L, size_t slices, int c, size_t K) {
  msm_slices<G>(sorted, kk, {px, py}, start, buckets, partial, broken, n, T, L, slices, c, K);
}
__global__ void __launch_bounds__(BLOCK) K_(combine)(const uint32_t* __restrict__ start, uint64_t* __restrict__ buckets, const uint64_t* __restrict__ partial,
                                                     uint32_t* __restrict__ broken, size_t L, size_t slices, int c, size_t K) {
  msm_combine<G>(start, buckets, partial, broken, L, slices, c, K);
}
__global__ void __launch_bounds__(BLOCK) K_(chunks)(const uint64_t* __restrict__ buckets, uint64_t* __restrict__ out, size_t lanes, size_t per_window, int c, int m, size_t K) {
  msm_chunks<G>(buckets, out, lanes, per_window, c, m, K);
}
__global__ void __launch_bounds__(BLOCK) K_(tree)(uint64_t* arr, size_t total, size_t count, size_t stride, size_t lanes, int fan) {
  msm_tree<G>(arr, total, count, stride, lanes, fan);
}
template <bool COMPRESSED>
__global__ void __launch_bounds__(BLOCK) K_(tree_affine)(const uint8_t* __restrict__ pts, uint32_t aligned, uint32_t* __restrict__ counter, uint64_t* __restrict__ out, size_t n,
                                                         size_t lanes, int fan) {
  const size_t g = (size_t)blockIdx.x * BLOCK + threadIdx.x;
  if (g >= lanes) return;
  G_(point) acc = G_(identity)();
#pragma unroll 1
  for (int t = 0; t < fan; ++t) {
    const size_t e = g + (size_t)t * lanes;
    if (e >= n) break;
    G_(affine) a;
    const int cls = COMPRESSED ? compressed_load(pts, e, aligned, a) : point_load(pts, e, aligned, a);
    if (cls == BLS381_MALFORMED) atomicAdd(counter, 1u);
    if (cls != BLS381_POINT) continue;
    acc = G_(madd)(acc, BLS381_Q2(a));
  }
  G::store(out, lanes, g, acc);
}
__global__ void __launch_bounds__(BLOCK) K_(products)(const uint64_t* __restrict__ k, const uint8_t* __restrict__ pts, uint32_t aligned, uint32_t* __restrict__ counter,
                                                      uint64_t* __restrict__ out, size_t n, int bits) {
  GID;
  G_(affine) a;
  const int cls = point_load(pts, i, aligned, a);
  if (cls == BLS381_MALFORMED) atomicAdd(counter, 1u);
  const fe kv = mask_bits(fe_load(k, i), bits);
  G::store(out, n, i, cls == BLS381_POINT ? G_(mul)(kv.w, a) : G_(identity)());
}
// One lane: msm_horner, then the uncompressed result.
__global__ void __launch_bounds__(64) K_(final)(const uint64_t* __restrict__ arr, size_t total, size_t stride, int windows, int c, const uint32_t* __restrict__ counter,
                                                uint8_t* __restrict__ out, uint32_t aligned, uint8_t* __restrict__ finite, uint32_t* __restrict__ invalid) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const G_(point) acc = msm_horner<G>(arr, total, stride, windows, c);
  const bool fin = !G_(is_identity)(acc);
  uint32_t bad = counter ? counter[0] : 0u;
  if (counter && counter[1] != 0u) {                                    // a broken invariant of the sort: no sum is better than a wrong one (ecsimd_msm.h, INTERNAL CHECK)
    fe381 ones;
#pragma unroll
    for (int j = 0; j < 12; ++j) ones.w[j] = 0xffffffffu;
    fill(out, 2 * NC, ones, aligned);
    bad = 0xffffffffu;
  } else jacobian_store(out, 0, aligned, acc);
  finite[0] = (uint8_t)((fin || bad == 0xffffffffu) ? 1 : 0);
  if (invalid) invalid[0] = bad;
}
}  // namespace

namespace launch {
static uint32_t word_aligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0 ? 1u : 0u; }
static dim3 grid_of(size_t lanes, size_t y = 1) { return dim3((unsigned)((lanes + BLOCK - 1) / BLOCK), (unsigned)y); }
using ML = BLS381_LAUNCH;
template <> void ML::decompress(hipStream_t s, const uint8_t* in, uint8_t* out, uint8_t* ok, size_t n) {
  hipLaunchKernelGGL(K_(decompress), grid_for(n), dim3(BLOCK), 0, s, in, word_aligned(in), out, word_aligned(out), ok, n);
}
template <> void ML::compress(hipStream_t s, const uint8_t* in, uint8_t* out, uint8_t* ok, size_t n) {
  hipLaunchKernelGGL(K_(compress), grid_for(n), dim3(BLOCK), 0, s, in, word_aligned(in), out, word_aligned(out), ok, n);
}
template <> void ML::check(hipStream_t s, const uint8_t* in, uint8_t* on_curve, uint8_t* in_subgroup, size_t n) {
  hipLaunchKernelGGL(K_(check), grid_for(n), dim3(BLOCK), 0, s, in, word_aligned(in), on_curve, in_subgroup, n);
}
template <> void ML::mul(hipStream_t s, const uint64_t* k, const uint8_t* in, uint8_t* out, uint8_t* ok, size_t n) {
  hipLaunchKernelGGL(K_(mul), grid_for(n), dim3(BLOCK), 0, s, k, in, word_aligned(in), out, word_aligned(out), ok, n);
}
template <> void ML::raw(hipStream_t s, int op, const uint8_t* in, uint8_t* out, size_t n) {
  hipLaunchKernelGGL(BLS381_K_RAW, grid_for(n), dim3(BLOCK), 0, s, op, in, out, word_aligned(in) & word_aligned(out), n);
}
template <> void ML::digits(hipStream_t s, const uint64_t* k, const uint8_t* pts, uint64_t* kk, uint64_t* px, uint64_t* py, uint32_t* hist, uint32_t* counter, size_t n, int bits, int c,
                            int windows) {
  hipLaunchKernelGGL(K_(digits), grid_of(n), dim3(BLOCK), 0, s, k, pts, word_aligned(pts), kk, px, py, hist, counter, n, bits, c, windows);
}
template <> void ML::slices(hipStream_t s, const uint32_t* sorted, const uint64_t* kk, const uint64_t* px, const uint64_t* py, const uint32_t* start, uint64_t* buckets,
                            uint64_t* partial, uint32_t* broken, size_t n, size_t T, size_t L, size_t slices, int c, size_t K) {
  hipLaunchKernelGGL(K_(slices), grid_of(slices), dim3(BLOCK), 0, s, sorted, kk, px, py, start, buckets, partial, broken, n, T, L, slices, c, K);
}
template <> void ML::combine(hipStream_t s, const uint32_t* start, uint64_t* buckets, const uint64_t* partial, uint32_t* broken, size_t L, size_t slices, int c, size_t K) {
  hipLaunchKernelGGL(K_(combine), grid_of(K), dim3(BLOCK), 0, s, start, buckets, partial, broken, L, slices, c, K);
}
template <> void ML::chunks(hipStream_t s, const uint64_t* buckets, uint64_t* out, size_t lanes, size_t per_window, int c, int m, size_t K) {
  hipLaunchKernelGGL(K_(chunks), grid_of(lanes), dim3(BLOCK), 0, s, buckets, out, lanes, per_window, c, m, K);
}
template <> void ML::tree(hipStream_t s, uint64_t* arr, size_t total, size_t count, size_t stride, size_t groups, size_t lanes, int fan) {
  hipLaunchKernelGGL(K_(tree), grid_of(lanes, groups), dim3(BLOCK), 0, s, arr, total, count, stride, lanes, fan);
}
template <> void ML::tree_affine(hipStream_t s, const uint8_t* pts, bool compressed, uint32_t* counter, uint64_t* out, size_t n, size_t lanes, int fan) {
  if (compressed) hipLaunchKernelGGL(K_(tree_affine)<true>, grid_of(lanes), dim3(BLOCK), 0, s, pts, word_aligned(pts), counter, out, n, lanes, fan);
  else hipLaunchKernelGGL(K_(tree_affine)<false>, grid_of(lanes), dim3(BLOCK), 0, s, pts, word_aligned(pts), counter, out, n, lanes, fan);
}
template <> void ML::products(hipStream_t s, const uint64_t* k, const uint8_t* pts, uint32_t* counter, uint64_t* out, size_t n, int bits) {
  hipLaunchKernelGGL(K_(products), grid_of(n), dim3(BLOCK), 0, s, k, pts, word_aligned(pts), counter, out, n, bits);
}
template <> void ML::finish(hipStream_t s, const uint64_t* arr, size_t total, size_t stride, int windows, int c, const uint32_t* counter, uint8_t* out, uint8_t* finite,
                            uint32_t* invalid) {
  hipLaunchKernelGGL(K_(final), dim3(1), dim3(64), 0, s, arr, total, stride, windows, c, counter, out, word_aligned(out), finite, invalid);
}
}  // namespace launch
}  // namespace ecsimd_hip
