// msm_stages.cuh -- the stages of the bucket method R = sum k_i P_i that do not depend on the group law, ONCE: the bodies behind the k_msm_* kernels of
// k_msm.inc (Weierstrass, Jacobian) and the k_edm_* kernels of k_msm_ed25519.hip (twisted Edwards, extended).  PUBLIC data only: bucket addresses are scalar
// digits.  The schedule -- which kernels, how many lanes, how long a lane's loop -- is a function of (n, bits, flags) alone (capi.hip msm_schedule_of,
// tools/msm_model.py); the data decide only which side of a branch a lane takes.
//
// T = n * windows entries, K = windows * 2^c keys (key = window * 2^c + digit).  In the order capi.hip's bucket_sum_run enqueues them:
//   zero       the two counters and the histogram, by a kernel (every node of a captured call is a kernel).  k_msm_common.hip.
//   digits     one lane per term: the unit validates or decodes the point and masks the scalar to `bits` bits (zeroed where the term contributes nothing);
//              msm_histogram takes the histogram of its c-bit digits, one vector atomic per window.
//   scan       one workgroup: the exclusive scan of the histogram -> start[K + 1], cursor[K].  k_msm_common.hip.
//   scatter    one lane per term: sorted[cursor[key]++] = i for every window (the order inside a bucket is whatever the atomics give: the sum commutes).
//              Every term has ONE entry per window, digit 0 included, so window w owns sorted[w n, (w + 1) n).  k_msm_common.hip.
//   slices     one lane per L consecutive entries of `sorted`: G::add_term into an accumulator, flushed where the key changes.  A run that holds its whole
//              bucket goes to the bucket; a run cut by the slice's edge goes to the slice's head slot (it starts at the slice's first entry) or tail slot (it
//              does not: then it runs to the slice's end).  At most L additions per lane.
//   combine    one lane per key: an empty bucket becomes the identity, a bucket spread over several slices the sum of their slots: at most
//              ceil(n / L) + 1 general additions, whatever the scalars (a bucket has at most n entries).
//   chunks     one lane per m buckets of a window: the running-sum form of sum t B_(j m + t) plus (j m) times the chunk's plain sum.
//   tree       fan-in 16 per launch, lanes owning strided slices; grid.y = the window.
//   final      one lane: msm_horner over the windows (c doublings each); what follows (the inversion or the encoding, the flag, the invalid count) is the unit's.
//
// A group policy G supplies: `point`; `terms`, the decoded terms' arrays as digits left them; identity(); add(P, Q) and dbl(P), for EVERY P and Q; add_term(P,
// terms, n, idx), P plus term idx; load / store(array, total, e, ...): element e of an array of G's planes of `total` elements each.
#pragma once
#include "kernels.h"
#include "field.cuh"

namespace ecsimd_hip {
// the low `bits` bits of k (1 <= bits <= 256)
ECS_DEV fe mask_bits(fe k, int bits) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int lo = 32 * j;
    if (bits <= lo) k.w[j] = 0u;
    else if (bits < lo + 32) k.w[j] &= (1u << (bits - lo)) - 1u;
  }
  return k;
}
// digit w of the masked scalar at kw (8 words in global memory: indexing registers by w would cost scratch), c <= 16 bits: at most two words
ECS_DEV uint32_t digit_of(const uint32_t* __restrict__ kw, int w, int c) {
  const int pos = w * c, word = pos >> 5, off = pos & 31;
  uint32_t v = kw[word] >> off;
  if (off + c > 32 && word < 7) v |= kw[word + 1] << (32 - off);
  return v & ((1u << c) - 1u);
}
// hist[w 2^c + digit w of kv] += 1 for every window.  The digits from the registers: a running 64-bit window over the words, shifted by c per step (no
// register is indexed by w)
ECS_DEV void msm_histogram(const fe& kv, uint32_t* __restrict__ hist, int c, int windows) {
  const uint32_t mask = (1u << c) - 1u;
  uint64_t acc = kv.w[0]; int have = 32, next = 1;
#pragma unroll 1
  for (int w = 0; w < windows; ++w) {
    if (have < c && next < 8) {
      uint32_t word = 0;
#pragma unroll
      for (int j = 1; j < 8; ++j) if (j == next) word = kv.w[j];
      acc |= (uint64_t)word << have; have += 32; ++next;
    }
    atomicAdd(&hist[((size_t)w << c) + ((uint32_t)acc & mask)], 1u);
    acc >>= c; have -= c;
  }
}

// where a finished run goes (see the head of the file); p0, p1 = the slice, first = the run's first entry in it
template <class G>
ECS_DEV void flush_run(uint32_t key, const typename G::point& acc, size_t first, size_t p0, size_t p1, size_t slice, const uint32_t* __restrict__ start, uint32_t dmask,
                       uint64_t* __restrict__ buckets, size_t K, uint64_t* __restrict__ partial, size_t slots) {
  if (key == 0xffffffffu || (key & dmask) == 0u) return;                // no run yet, or digit 0: skipped
  const size_t a = start[key], b = start[key + 1];
  if (a >= p0 && b <= p1) G::store(buckets, K, key, acc);
  else G::store(partial, slots, 2 * slice + (first == p0 ? 0 : 1), acc);
}
template <class G>
ECS_DEV void msm_slices(const uint32_t* __restrict__ sorted, const uint64_t* __restrict__ kk, const typename G::terms& terms, const uint32_t* __restrict__ start,
                        uint64_t* __restrict__ buckets, uint64_t* __restrict__ partial, uint32_t* __restrict__ broken, size_t n, size_t T, size_t L, size_t slices, int c, size_t K) {
  const size_t s = (size_t)blockIdx.x * launch::BLOCK + threadIdx.x;
  if (s >= slices) return;
  const size_t p0 = s * L, p1 = p0 + L < T ? p0 + L : T;
  const uint32_t dmask = (1u << c) - 1u;
  int w = (int)(p0 / n);
  size_t wend = ((size_t)w + 1) * n, first = p0;
  uint32_t cur = 0xffffffffu;
  typename G::point acc = G::identity();
#pragma unroll 1
  for (size_t pos = p0; pos < p1; ++pos) {
    while (pos >= wend) { ++w; wend += n; }
    const size_t idx = sorted[pos];
    if (idx >= n) { atomicAdd(broken, 1u); continue; }                  // every entry was written by the scatter: anything else fails the call
    const uint32_t d = digit_of(reinterpret_cast<const uint32_t*>(kk) + 8 * idx, w, c);
    const uint32_t key = ((uint32_t)w << c) + d;
    if (key != cur) {
      flush_run<G>(cur, acc, first, p0, p1, s, start, dmask, buckets, K, partial, 2 * slices);
      cur = key; first = pos; acc = G::identity();
    }
    if (d != 0u) acc = G::add_term(acc, terms, n, idx);                 // (digit 0 goes to no bucket: skipping it is the schedule's, not the group law's)
  }
  flush_run<G>(cur, acc, first, p0, p1, s, start, dmask, buckets, K, partial, 2 * slices);
}

template <class G>
ECS_DEV void msm_combine(const uint32_t* __restrict__ start, uint64_t* __restrict__ buckets, const uint64_t* __restrict__ partial, uint32_t* __restrict__ broken, size_t L,
                         size_t slices, int c, size_t K) {
  const size_t key = (size_t)blockIdx.x * launch::BLOCK + threadIdx.x;
  if (key >= K || (key & ((1u << c) - 1u)) == 0) return;
  const size_t a = start[key], b = start[key + 1];
  if (a > b || b > slices * L) atomicAdd(broken, 1u);                  // offsets that are no scan of a histogram fail the call; no load follows them out of `partial`
  if (a >= b || b > slices * L) { G::store(buckets, K, key, G::identity()); return; }     // a == b: an empty bucket
  const size_t s0 = a / L, s1 = (b - 1) / L;
  if (s0 == s1) return;                                                 // the whole bucket lay in one slice, which wrote it
  typename G::point acc = G::identity();
#pragma unroll 1
  for (size_t s = s0; s <= s1; ++s) acc = G::add(acc, G::load(partial, 2 * slices, 2 * s + (a <= s * L ? 0 : 1)));
  G::store(buckets, K, key, acc);
}

// lane (w, j): sum over t < m of (j m + t) B[j m + t] = sum t B + (j m) sum B.  Bucket 0 of a window is never read.
template <class G>
ECS_DEV void msm_chunks(const uint64_t* __restrict__ buckets, uint64_t* __restrict__ out, size_t lanes, size_t per_window, int c, int m, size_t K) {
  const size_t g = (size_t)blockIdx.x * launch::BLOCK + threadIdx.x;
  if (g >= lanes) return;
  const size_t w = g / per_window, j = g % per_window, off = j * (size_t)m, base = (w << c) + off;
  typename G::point run = G::identity(), tot = G::identity();
#pragma unroll 1
  for (int t = m - 1; t >= 0; --t) {
    if (off + t != 0) run = G::add(run, G::load(buckets, K, base + t));
    if (t != 0) tot = G::add(tot, run);
  }
  typename G::point mult = G::identity();
#pragma unroll 1
  for (int bit = c - 1; bit >= 0; --bit) {
    mult = G::dbl(mult);
    if ((off >> bit) & 1u) mult = G::add(mult, run);
  }
  G::store(out, lanes, g, G::add(tot, mult));
}

// arr[group * stride + g] = the sum of arr[group * stride + g + t * lanes], t < fan, for g < lanes: in place (a lane reads its own elements, then writes the first)
template <class G>
ECS_DEV void msm_tree(uint64_t* arr, size_t total, size_t count, size_t stride, size_t lanes, int fan) {
  const size_t g = (size_t)blockIdx.x * launch::BLOCK + threadIdx.x;
  if (g >= lanes) return;
  const size_t base = (size_t)blockIdx.y * stride;
  typename G::point acc = G::load(arr, total, base + g);
#pragma unroll 1
  for (int t = 1; t < fan; ++t) {
    const size_t e = g + (size_t)t * lanes;
    if (e >= count) break;
    acc = G::add(acc, G::load(arr, total, base + e));
  }
  G::store(arr, total, base + g, acc);
}

// windows > 0: arr[w * stride] = the sum of window w; Horner from the top, c doublings per window.  windows == 0: the empty sum.
template <class G>
ECS_DEV typename G::point msm_horner(const uint64_t* __restrict__ arr, size_t total, size_t stride, int windows, int c) {
  typename G::point acc = G::identity();
#pragma unroll 1
  for (int w = windows - 1; w >= 0; --w) {
#pragma unroll 1
    for (int d = 0; d < c; ++d) acc = G::dbl(acc);
    acc = G::add(acc, G::load(arr, total, (size_t)w * stride));
  }
  return acc;
}
}  // namespace ecsimd_hip
