// ntt.cuh -- the number-theoretic transform's schedule, index arithmetic and pass body (include/ecsimd_ntt.h), written so that it also compiles for the HOST.
//
// Nothing here includes a device-only header: the schedule is what ecsimd_ntt_plan reports, and tests/cpp/ntt_host_check.cpp runs the pass body lane by lane on a
// CPU over the portable field below.  k_ntt.hip instantiates the same body over gfield.cuh's g_add / g_sub / g_mul.
//
// THE TRANSFORM.  n = 2^L elements, split into P passes of log-radix R_1 .. R_P (sum L).  It is the Stockham self-sorting form: natural order in, natural order
// out, no bit reversal between passes.  Before pass i let s = 2^(R_1 + .. + R_(i-1)) and r = 2^R_i.  The array is a matrix of r rows and n / r COLUMNS:
//     column c, row j  is read at   c + j (n / r)                                  -- the same pattern in every pass
//     output k of it   is written at  q + s k + s r p,  q = c mod s, p = c div s   -- times omega^(s p k) unless the pass is the last (p = 0 there)
// A pass reads one buffer and writes another; the LAST pass writes the places it read, so it may run in place.  A batch is one long run of columns: column
// C = b (n / r) + c of transform b.  A workgroup takes T = 2^(TILE_LOG - R_i) consecutive columns -- a TILE of 2^TILE_LOG elements --, so that it reads runs of
// T >= 4 consecutive elements (or, where n / r < T, whole small transforms), and writes runs of max(T, r s) or of T.
//
// LDS.  An element is two 16-byte halves in two PLANES; plane h holds half h of element (row, column) in 16-byte slot row (T + 1) + column.  A wave's
// ds_read_b128 is served in groups of 16 lanes, 256 bytes = all 64 banks per group when the 16 slots are distinct modulo 16: a run along a row is, and so is a walk
// down a column, because the row stride T + 1 is odd (DESIGN.md section 4p has the cases that are not).  Rows hold the inputs in BIT-REVERSED order; R_i stages of
// decimation-in-time butterflies leave the outputs in natural order.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define NTT_HD __host__ __device__ __forceinline__
#else
#define NTT_HD inline
#endif

namespace ecsimd_hip {
namespace ntt {

constexpr int TILE_LOG = 11;                         // elements a workgroup holds: 2^11 x 32 B = 64 KiB (+ the row padding)
constexpr int TILE = 1 << TILE_LOG;
constexpr int LANES = 256;                           // 8 elements and 4 butterflies per lane and stage
constexpr int DEFAULT_RADIX_LOG = 9;                 // the largest log-radix of a pass: leaves T >= 4 columns in a tile
constexpr int MAX_LOG_N = 24;
constexpr int MAX_PASSES = MAX_LOG_N;                // ECSIMD_NTT_MAX_RADIX_LOG(1): one stage per pass
constexpr int SPLIT_LOG = 12;                        // the two-level tables: x^i = lo[i mod 2^12] * hi[i div 2^12]
constexpr int SPLIT = 1 << SPLIT_LOG;
constexpr int PLANE_SLOTS = TILE + (1 << DEFAULT_RADIX_LOG);    // rows (T + 1) = TILE + r <= this
constexpr int LDS_SLOTS = 2 * PLANE_SLOTS;
constexpr int LDS_BYTES = LDS_SLOTS * 16;            // 81 920: two workgroups per CU

struct u4 { alignas(16) uint32_t v[4]; };            // a 16-byte half element: what one dwordx4 / ds_*_b128 moves

// ---- the schedule: a function of (log_n, cap) alone
struct schedule { int passes; int log_radix[MAX_PASSES]; };
// cap in 1 .. DEFAULT_RADIX_LOG.  The fewest passes the cap allows, the stages spread evenly, the wider passes first.
NTT_HD bool make_schedule(int log_n, int cap, schedule* S) {
  if (log_n < 1 || log_n > MAX_LOG_N || cap < 1 || cap > DEFAULT_RADIX_LOG) return false;
  const int P = (log_n + cap - 1) / cap, base = log_n / P, rem = log_n % P;
  S->passes = P;
  for (int i = 0; i < MAX_PASSES; ++i) S->log_radix[i] = i < P ? base + (i < rem ? 1 : 0) : 0;
  return true;
}
// Which buffer pass i (0-based) writes: 1 = the workspace, 0 = out.  The input may BE out, so the first pass of several goes to the workspace; the passes
// alternate from there; the last writes out -- in place when the one before it did too (an odd number of passes), which the last pass alone may.
NTT_HD int pass_writes_workspace(int i, int passes) { return i + 1 < passes && (i & 1) == 0; }

// ---- one pass's geometry
struct geom {
  int log_n, log_r, log_s;      // n, this pass's radix, the product of the radices before it
  int log_t, log_w;             // columns in a tile (TILE_LOG - log_r) and in a transform (log_n - log_r)
  int log_rt;                   // the stage table holds omega_(2^log_rt)^i, i < 2^(log_rt - 1): log_rt = min(log_n, DEFAULT_RADIX_LOG)
  int first, last, inverse, coset;
  uint64_t columns;             // batch << log_w
};
NTT_HD geom make_geom(int log_n, const schedule& S, int pass, uint64_t batch, int inverse, int coset) {
  geom G;
  G.log_n = log_n; G.log_r = S.log_radix[pass]; G.log_s = 0;
  for (int i = 0; i < pass; ++i) G.log_s += S.log_radix[i];
  G.log_t = TILE_LOG - G.log_r; G.log_w = log_n - G.log_r;
  G.log_rt = log_n < DEFAULT_RADIX_LOG ? log_n : DEFAULT_RADIX_LOG;
  G.first = pass == 0; G.last = pass + 1 == S.passes; G.inverse = inverse; G.coset = coset;
  G.columns = batch << G.log_w;
  return G;
}
NTT_HD uint64_t tiles_of(const geom& G) { return (G.columns + ((uint64_t)1 << G.log_t) - 1) >> G.log_t; }

NTT_HD uint32_t bitrev(uint32_t v, int bits) {          // 1 <= bits <= 32
#if defined(__HIP_DEVICE_COMPILE__)
  return __brev(v) >> (32 - bits);
#endif
  uint32_t r = 0;
  for (int i = 0; i < bits; ++i) r |= ((v >> i) & 1u) << (bits - 1 - i);
  return r;
}
// column C of the batch: its transform b and its column c in it
NTT_HD uint64_t col_batch(const geom& G, uint64_t C) { return C >> G.log_w; }
NTT_HD uint32_t col_in_transform(const geom& G, uint64_t C) { return (uint32_t)(C & (((uint64_t)1 << G.log_w) - 1)); }
// where row j of column C is read, and its index in its transform (the exponent of the coset's g^i)
NTT_HD uint32_t src_index(const geom& G, uint32_t c, uint32_t j) { return c + (j << G.log_w); }
// where output k of column c is written (in its transform), and the exponent of the twiddle it takes first
NTT_HD uint32_t dst_index(const geom& G, uint32_t c, uint32_t k) {
  const uint32_t q = c & ((1u << G.log_s) - 1), p = c >> G.log_s;
  return q + (k << G.log_s) + (p << (G.log_s + G.log_r));
}
NTT_HD uint32_t twiddle_exponent(const geom& G, uint32_t c, uint32_t k) { return ((c >> G.log_s) * k) << G.log_s; }      // s p k < n
// The order in which a tile's lanes walk its elements, chosen for runs in global memory.  o in [0, TILE) -> (column t of the tile, row).
// load: along the columns where a transform has a tile's worth of them, else through each small transform's rows as they lie in memory.
NTT_HD void load_order(const geom& G, uint32_t o, uint32_t* t, uint32_t* j) {
  if (G.log_w >= G.log_t) { *t = o & ((1u << G.log_t) - 1); *j = o >> G.log_t; return; }
  const uint32_t c = o & ((1u << G.log_w) - 1), b = o >> G.log_n;
  *j = (o >> G.log_w) & ((1u << G.log_r) - 1);
  *t = (b << G.log_w) | c;
}
// store: along the columns where s covers a tile's columns, else along q, then k, then p -- the order of the addresses q + s k + s r p
NTT_HD void store_order(const geom& G, uint32_t o, uint32_t* t, uint32_t* k) {
  if (G.log_s >= G.log_t) { *t = o & ((1u << G.log_t) - 1); *k = o >> G.log_t; return; }
  const uint32_t q = o & ((1u << G.log_s) - 1), ph = o >> (G.log_s + G.log_r);
  *k = (o >> G.log_s) & ((1u << G.log_r) - 1);
  *t = (ph << G.log_s) | q;
}
// butterfly h (of r / 2) of stage u: rows j0 and j0 + 2^u, and the index of omega_(2^(u+1))^(j0 mod 2^u) in the stage table
NTT_HD void butterfly_rows(const geom& G, uint32_t h, int u, uint32_t* j0, uint32_t* tw) {
  const uint32_t low = h & ((1u << u) - 1);
  *j0 = ((h >> u) << (u + 1)) | low;
  *tw = low << (G.log_rt - 1 - u);
}
NTT_HD uint32_t lds_slot(const geom& G, uint32_t row, uint32_t t) { return row * ((1u << G.log_t) + 1) + t; }

// ---- the domain's tables, all in Montgomery form unless said otherwise, for the direction of the call
struct tables {
  const u4* stage;      // omega_(2^log_rt)^(+-i), i < 2^(log_rt - 1)
  const u4* lo;         // omega^(+-i), i < min(n, SPLIT)
  const u4* hi;         // omega^(+-SPLIT i), i < max(1, n / SPLIT)
  const u4* glo;        // forward: g^i;  inverse: g^-i                         (i < min(n, SPLIT))
  const u4* ghi;        // forward: g^(SPLIT i) R^2, so that x * (glo * ghi) = x g^i R;  inverse: n^-1 g^(-SPLIT i) CLASSICAL, so that (y R) * (glo * ghi) = y n^-1 g^-i
};
struct pass_args { const u4* src; u4* dst; tables tw; geom G; };

// ---- the pass body, one phase per function; a workgroup (or the host check) runs a phase for every lane, then the next.  F is the field:
//   F::el, el load(u4, u4), void store(el, u4*, u4*), el add(el, el), el sub(el, el), el mul(el, el) [Montgomery product], el rsq(), el one()
template <class F> NTT_HD typename F::el table_at(const F& f, const u4* t, uint32_t i) { return f.load(t[2 * (size_t)i], t[2 * (size_t)i + 1]); }
template <class F> NTT_HD typename F::el split_power(const F& f, const geom& G, const u4* lo, const u4* hi, uint32_t e) {
  typename F::el v = table_at(f, lo, e & (SPLIT - 1));
  if (G.log_n > SPLIT_LOG) v = f.mul(v, table_at(f, hi, e >> SPLIT_LOG));
  return v;
}
constexpr int LOAD_GROUP = 4;       // global loads a lane has in flight before it multiplies

// global -> LDS: to Montgomery form (and, forward, onto the coset: times g^i) in the first pass, rows bit-reversed
template <class F> NTT_HD void pass_load(const F& f, const pass_args& A, uint64_t tile, int lane, u4* lds) {
  const geom& G = A.G;
  const uint64_t C0 = tile << G.log_t;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
  for (int it = 0; it < TILE / LANES; it += LOAD_GROUP) {
    u4 raw[LOAD_GROUP][2]; uint32_t slot[LOAD_GROUP], idx[LOAD_GROUP]; bool live[LOAD_GROUP];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int g = 0; g < LOAD_GROUP; ++g) {
      uint32_t t, j;
      load_order(G, (uint32_t)lane + (uint32_t)(it + g) * LANES, &t, &j);
      const uint64_t C = C0 + t;
      live[g] = C < G.columns;
      const uint32_t c = col_in_transform(G, C);
      idx[g] = src_index(G, c, j);
      slot[g] = lds_slot(G, bitrev(j, G.log_r), t);
      if (live[g]) {
        const size_t e = ((size_t)col_batch(G, C) << G.log_n) + idx[g];
        raw[g][0] = A.src[2 * e]; raw[g][1] = A.src[2 * e + 1];
      }
    }
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int g = 0; g < LOAD_GROUP; ++g) {
      if (!live[g]) continue;
      typename F::el v = f.load(raw[g][0], raw[g][1]);
      if (G.first) v = f.mul(v, G.coset && !G.inverse ? f.mul(table_at(f, A.tw.glo, idx[g] & (SPLIT - 1)), table_at(f, A.tw.ghi, idx[g] >> SPLIT_LOG)) : f.rsq());
      f.store(v, &lds[slot[g]], &lds[PLANE_SLOTS + slot[g]]);
    }
  }
}
// stage u: (a, b) -> (a + w b, a - w b) on rows j0, j0 + 2^u of every column
template <class F> NTT_HD void pass_stage(const F& f, const pass_args& A, uint64_t tile, int lane, int u, u4* lds) {
  const geom& G = A.G;
  const uint64_t C0 = tile << G.log_t;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
  for (int it = 0; it < TILE / 2 / LANES; ++it) {
    const uint32_t b = (uint32_t)lane + (uint32_t)it * LANES, t = b & ((1u << G.log_t) - 1);
    if (C0 + t >= G.columns) continue;
    uint32_t j0, tw;
    butterfly_rows(G, b >> G.log_t, u, &j0, &tw);
    const uint32_t s0 = lds_slot(G, j0, t), s1 = lds_slot(G, j0 + (1u << u), t);
    const typename F::el x = f.load(lds[s0], lds[PLANE_SLOTS + s0]);
    typename F::el y = f.load(lds[s1], lds[PLANE_SLOTS + s1]);
    if (u > 0) y = f.mul(y, table_at(f, A.tw.stage, tw));                  // stage 0's twiddle is 1
    f.store(f.add(x, y), &lds[s0], &lds[PLANE_SLOTS + s0]);
    f.store(f.sub(x, y), &lds[s1], &lds[PLANE_SLOTS + s1]);
  }
}
// LDS -> global: times omega^(s p k) between passes; out of Montgomery form (times n^-1 g^-i on the inverse) in the last
template <class F> NTT_HD void pass_store(const F& f, const pass_args& A, uint64_t tile, int lane, const u4* lds) {
  const geom& G = A.G;
  const uint64_t C0 = tile << G.log_t;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
  for (int it = 0; it < TILE / LANES; ++it) {
    uint32_t t, k;
    store_order(G, (uint32_t)lane + (uint32_t)it * LANES, &t, &k);
    const uint64_t C = C0 + t;
    if (C >= G.columns) continue;
    const uint32_t c = col_in_transform(G, C), i = dst_index(G, c, k), s = lds_slot(G, k, t);
    typename F::el v = f.load(lds[s], lds[PLANE_SLOTS + s]);
    if (!G.last) v = f.mul(v, split_power(f, G, A.tw.lo, A.tw.hi, twiddle_exponent(G, c, k)));
    else if (!G.inverse) v = f.mul(v, f.one());
    else v = f.mul(v, G.coset ? f.mul(table_at(f, A.tw.glo, i & (SPLIT - 1)), table_at(f, A.tw.ghi, i >> SPLIT_LOG)) : table_at(f, A.tw.ghi, 0));
    const size_t e = ((size_t)col_batch(G, C) << G.log_n) + i;
    f.store(v, &A.dst[2 * e], &A.dst[2 * e + 1]);
  }
}

// ---- the portable field: Montgomery arithmetic on eight 32-bit words in plain C++, canonical results like gfield.cuh's.  The host builds the domain's tables with
// it and the host check runs the passes over it.
struct pel { uint32_t w[8]; };
struct pfield {
  typedef pel el;
  uint32_t p[8], r2[8], mprime;
  NTT_HD static pel load(const u4& a, const u4& b) { pel r; for (int i = 0; i < 4; ++i) { r.w[i] = a.v[i]; r.w[4 + i] = b.v[i]; } return r; }
  NTT_HD static void store(const pel& v, u4* a, u4* b) { for (int i = 0; i < 4; ++i) { a->v[i] = v.w[i]; b->v[i] = v.w[4 + i]; } }
  NTT_HD pel rsq() const { pel r; for (int i = 0; i < 8; ++i) r.w[i] = r2[i]; return r; }
  NTT_HD static pel one() { pel r; for (int i = 0; i < 8; ++i) r.w[i] = i == 0; return r; }
  NTT_HD void cond_sub(pel& r, uint32_t top) const {                       // r + top 2^256 < 2 p  ->  mod p
    uint32_t d[8]; uint64_t bw = 0;
    for (int i = 0; i < 8; ++i) { const uint64_t x = (uint64_t)r.w[i] - p[i] - bw; d[i] = (uint32_t)x; bw = (x >> 32) & 1u; }
    if (top || !bw) for (int i = 0; i < 8; ++i) r.w[i] = d[i];
  }
  NTT_HD pel add(const pel& a, const pel& b) const {
    pel r; uint64_t c = 0;
    for (int i = 0; i < 8; ++i) { c += (uint64_t)a.w[i] + b.w[i]; r.w[i] = (uint32_t)c; c >>= 32; }
    cond_sub(r, (uint32_t)c);
    return r;
  }
  NTT_HD pel sub(const pel& a, const pel& b) const {
    pel r; uint64_t bw = 0;
    for (int i = 0; i < 8; ++i) { const uint64_t x = (uint64_t)a.w[i] - b.w[i] - bw; r.w[i] = (uint32_t)x; bw = (x >> 32) & 1u; }
    if (bw) { uint64_t c = 0; for (int i = 0; i < 8; ++i) { c += (uint64_t)r.w[i] + p[i]; r.w[i] = (uint32_t)c; c >>= 32; } }
    return r;
  }
  // a b 2^-256 mod p for a < 2^256, b < p (word-serial, operand scanning)
  NTT_HD pel mul(const pel& a, const pel& b) const {
    uint32_t t[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int i = 0; i < 8; ++i) {
      uint64_t c = 0;
      for (int j = 0; j < 8; ++j) { c += (uint64_t)t[j] + (uint64_t)a.w[j] * b.w[i]; t[j] = (uint32_t)c; c >>= 32; }
      c += t[8]; t[8] = (uint32_t)c; t[9] = (uint32_t)(c >> 32);
      const uint32_t q = t[0] * mprime;
      c = ((uint64_t)t[0] + (uint64_t)q * p[0]) >> 32;
      for (int j = 1; j < 8; ++j) { c += (uint64_t)t[j] + (uint64_t)q * p[j]; t[j - 1] = (uint32_t)c; c >>= 32; }
      c += t[8]; t[7] = (uint32_t)c; t[8] = t[9] + (uint32_t)(c >> 32);
    }
    pel r; for (int i = 0; i < 8; ++i) r.w[i] = t[i];
    cond_sub(r, t[8]);
    return r;
  }
};

}  // namespace ntt
}  // namespace ecsimd_hip
