// ed25519.cuh -- the twisted Edwards curve -x^2 + y^2 = 1 + d x^2 y^2 over 2^255 - 19 in extended coordinates (X, Y, Z, T), x = X / Z, y = Y / Z, x y = T / Z.
//
// a = -1 is a square and d is not, so the unified addition (Hisil, Wong, Carter, Dawson 2008) is COMPLETE: the same formula for P + Q, P + P, P + (-P) and
// P + identity, no exceptional case to select around and none to leak.  Three shapes of a second operand:
//   * ed_point   (X, Y, Z, T);
//   * ed_cached  (Y + X, Y - X, Z, 2 d T): a per-lane table entry of the verification loop (8 M per addition);
//   * ed_precomp (y + x, y - x, 2 d x y), Z = 1: an entry of the shared table of multiples of B (7 M).
// The doubling is the dedicated one (4 S + 4 M); inside a run of doublings T is not needed and is not computed (ed_dbl_nt, 4 S + 3 M).
//
// Two scalar-multiplication loops, both on scalars already below L (gfield.cuh's Montgomery arithmetic with L as the modulus reduces them):
//   * ed_base_ct     [k]B for SECRET k: a comb over ED25519_BASE (32 rows of 1 .. 8 times 256^i B).  k + 0x88...8 cut into 64 nibbles gives the signed digits
//                    nibble - 8 in [-8, 7] without a carry chain or a branch; the odd positions are summed first, four doublings, then the even ones
//                    (64 mixed additions, 4 doublings).  EVERY entry of a row is read, at addresses that depend on the row alone, and chosen by masks;
//                    the sign is a masked swap and negation.
//   * ed_straus_vartime  [s]B + [h]P for PUBLIC data: one loop over the same signed digits of both scalars, four shared doublings per position, B's multiples
//                    from row 0 of the shared table, P's from a per-lane table of 1 .. 8 times P in memory.  INDEXED BY THE DIGITS AND BRANCHING ON THEM:
//                    NOT FOR SECRETS.
#pragma once
#include "fe25519.cuh"
#include "gfield.cuh"

namespace ecsimd_hip {

struct ed_point { fe X, Y, Z, T; };
struct ed_cached { fe YpX, YmX, Z, T2d; };
struct ed_precomp { fe ypx, ymx, xy2d; };

__device__ const uint32_t ED25519_BASE[32 * 8 * 24] = {ED25519_BASE_TABLE};

ECS_DEV ed_point ed_identity() { return {fe25519_small(0u), fe25519_small(1u), fe25519_small(1u), fe25519_small(0u)}; }
ECS_DEV ed_point ed_neg(const ed_point& p) { return {fe25519_neg(p.X), p.Y, p.Z, fe25519_neg(p.T)}; }
ECS_DEV ed_cached ed_to_cached(const ed_point& p) {
  return {fe25519_add(p.Y, p.X), fe25519_sub(p.Y, p.X), p.Z, fe25519_mul(p.T, fe25519_const<ed25519_consts::D2>())};
}
// (E, F, G, H) -> X = E F, Y = G H, Z = F G, T = E H
ECS_DEV ed_point ed_complete(const fe& E, const fe& F, const fe& G, const fe& H) {
  return {fe25519_mul(E, F), fe25519_mul(G, H), fe25519_mul(F, G), fe25519_mul(E, H)};
}
ECS_DEV ed_point ed_add_cached(const ed_point& p, const ed_cached& q) {
  const fe A = fe25519_mul(fe25519_sub(p.Y, p.X), q.YmX), B = fe25519_mul(fe25519_add(p.Y, p.X), q.YpX);
  const fe C = fe25519_mul(p.T, q.T2d), Z = fe25519_mul(p.Z, q.Z), D = fe25519_add(Z, Z);
  return ed_complete(fe25519_sub(B, A), fe25519_sub(D, C), fe25519_add(D, C), fe25519_add(B, A));
}
ECS_DEV ed_point ed_add(const ed_point& p, const ed_point& q) { return ed_add_cached(p, ed_to_cached(q)); }
ECS_DEV ed_point ed_add_precomp(const ed_point& p, const ed_precomp& q) {
  const fe A = fe25519_mul(fe25519_sub(p.Y, p.X), q.ymx), B = fe25519_mul(fe25519_add(p.Y, p.X), q.ypx);
  const fe C = fe25519_mul(p.T, q.xy2d), D = fe25519_add(p.Z, p.Z);
  return ed_complete(fe25519_sub(B, A), fe25519_sub(D, C), fe25519_add(D, C), fe25519_add(B, A));
}
// A = X^2, B = Y^2, C = 2 Z^2, H = A + B, E = H - (X + Y)^2, G = A - B, F = C + G
#define ED_DBL_EFGH(p) \
  const fe A_ = fe25519_sqr((p).X), B_ = fe25519_sqr((p).Y), Z2_ = fe25519_sqr((p).Z), C_ = fe25519_add(Z2_, Z2_); \
  const fe H_ = fe25519_add(A_, B_), E_ = fe25519_sub(H_, fe25519_sqr(fe25519_add((p).X, (p).Y))), G_ = fe25519_sub(A_, B_), F_ = fe25519_add(C_, G_)
ECS_DEV ed_point ed_dbl(const ed_point& p) { ED_DBL_EFGH(p); return ed_complete(E_, F_, G_, H_); }
// the same without T (left as it was: the next operation must be a doubling)
ECS_DEV void ed_dbl_nt(ed_point& p) { ED_DBL_EFGH(p); p.X = fe25519_mul(E_, F_); p.Y = fe25519_mul(G_, H_); p.Z = fe25519_mul(F_, G_); }
#undef ED_DBL_EFGH
// p * 16
ECS_DEV ed_point ed_dbl4(ed_point p) {
  ed_dbl_nt(p); ed_dbl_nt(p); ed_dbl_nt(p);
  return ed_dbl(p);
}

// ---- the wire format: 32 bytes little-endian, y in bits 0 .. 254, the parity of x in bit 255.  As words: fe.w[j] = bytes 4 j .. 4 j + 3.
ECS_DEV fe ed_load32(const uint8_t* __restrict__ p, uint32_t aligned) {
  fe r;
  if (aligned) {
    const uint32_t* q = reinterpret_cast<const uint32_t*>(p);
#pragma unroll
    for (int j = 0; j < 8; ++j) r.w[j] = q[j];
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) r.w[j] = (uint32_t)p[4 * j] | ((uint32_t)p[4 * j + 1] << 8) | ((uint32_t)p[4 * j + 2] << 16) | ((uint32_t)p[4 * j + 3] << 24);
  }
  return r;
}
ECS_DEV void ed_store32(uint8_t* __restrict__ p, const fe& v, uint32_t aligned) {
  if (aligned) {
    uint32_t* q = reinterpret_cast<uint32_t*>(p);
#pragma unroll
    for (int j = 0; j < 8; ++j) q[j] = v.w[j];
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) { p[4 * j] = (uint8_t)v.w[j]; p[4 * j + 1] = (uint8_t)(v.w[j] >> 8); p[4 * j + 2] = (uint8_t)(v.w[j] >> 16); p[4 * j + 3] = (uint8_t)(v.w[j] >> 24); }
  }
}
// one inversion
ECS_DEV fe ed_encode(const ed_point& p) {
  const fe zi = fe25519_invert(p.Z);
  const fe x = fe25519_canon(fe25519_mul(p.X, zi));
  fe y = fe25519_canon(fe25519_mul(p.Y, zi));
  y.w[7] |= x.w[0] << 31;
  return y;
}
// all ones where the encoding is a point: y < p, x^2 = (y^2 - 1) / (d y^2 + 1) has a root, and not (x = 0 with the sign bit set).  p is the point where it
// is one and (the chain's leftovers, y, 1, ..) where not: a caller masks by the result.
ECS_DEV uint32_t ed_decode(ed_point& p, const fe& enc) {
  fe y = enc;
  const uint32_t sign = y.w[7] >> 31;
  y.w[7] &= 0x7fffffffu;
  const fe yc = fe25519_canon(y);
  uint32_t diff = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) diff |= yc.w[i] ^ y.w[i];
  const uint32_t canonical = (uint32_t)((int32_t)((diff | (0u - diff)) ^ 0x80000000u) >> 31);
  const fe yy = fe25519_sqr(y), one = fe25519_small(1u);
  const fe u = fe25519_sub(yy, one), v = fe25519_add(fe25519_mul(yy, fe25519_const<ed25519_consts::D>()), one);
  fe x;
  const uint32_t root = fe25519_sqrt_ratio(x, u, v);
  x = fe25519_canon(x);
  const uint32_t zero_signed = fe25519_zero_mask(x) & (0u - sign);
  x = fe25519_select(0u - ((x.w[0] & 1u) ^ sign), fe25519_neg(x), x);
  p.X = x; p.Y = y; p.Z = one; p.T = fe25519_mul(x, y);
  return canonical & root & ~zero_signed;
}

// ---- signed radix-16 digits of k < 2^253: nibble i of k + 0x88...8, minus 8
ECS_DEV fe ed_digits_of(const fe& k) {
  fe b, r;
#pragma unroll
  for (int i = 0; i < 8; ++i) b.w[i] = 0x88888888u;
  (void)add8m3(r, k, b);                                         // k < 2^253: no carry out
  return r;
}
// The loops never index the words by position (a variable index would put them in scratch memory or LDS): they read the digit at one end and shift.
ECS_DEV void ed_shr8(fe& v) {
#pragma unroll
  for (int j = 0; j < 7; ++j) v.w[j] = __builtin_amdgcn_alignbit(v.w[j + 1], v.w[j], 8);
  v.w[7] >>= 8;
}
ECS_DEV void ed_shl4(fe& v) {
#pragma unroll
  for (int j = 7; j > 0; --j) v.w[j] = __builtin_amdgcn_alignbit(v.w[j], v.w[j - 1], 28);
  v.w[0] <<= 4;
}

// ---- [k]B for SECRET k < L
ECS_DEV ed_precomp ed_base_select_ct(int row, int32_t digit) {
  const uint32_t neg = (uint32_t)(digit >> 31), mag = ((uint32_t)digit ^ neg) - neg;      // |digit| in 0 .. 8
  ed_precomp e = {fe25519_small(1u), fe25519_small(1u), fe25519_small(0u)};                // the identity: digit 0
  const uint32_t* t = ED25519_BASE + row * (8 * 24);
#pragma unroll
  for (uint32_t j = 1; j <= 8; ++j) {
    const uint32_t d = mag ^ j;
    const uint32_t m = (uint32_t)((int32_t)((d | (0u - d)) ^ 0x80000000u) >> 31);         // all ones where |digit| = j
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      e.ypx.w[q] = (t[(j - 1) * 24 + q] & m) | (e.ypx.w[q] & ~m);
      e.ymx.w[q] = (t[(j - 1) * 24 + 8 + q] & m) | (e.ymx.w[q] & ~m);
      e.xy2d.w[q] = (t[(j - 1) * 24 + 16 + q] & m) | (e.xy2d.w[q] & ~m);
    }
  }
  const ed_precomp n = {e.ymx, e.ypx, fe25519_neg(e.xy2d)};                                // the negative: swap, and - 2 d x y
  return {fe25519_select(neg, n.ypx, e.ypx), fe25519_select(neg, n.ymx, e.ymx), fe25519_select(neg, n.xy2d, e.xy2d)};
}
ECS_DEV ed_point ed_base_ct(const fe& k) {
  const fe biased = ed_digits_of(k);
  ed_point p = ed_identity();
  fe cur = biased;
#pragma unroll 1
  for (int row = 0; row < 32; ++row) {                           // positions 1, 3, .. 63
    p = ed_add_precomp(p, ed_base_select_ct(row, (int32_t)((cur.w[0] >> 4) & 15u) - 8));
    ed_shr8(cur);
  }
  p = ed_dbl4(p);
  cur = biased;
#pragma unroll 1
  for (int row = 0; row < 32; ++row) {                           // positions 0, 2, .. 62
    p = ed_add_precomp(p, ed_base_select_ct(row, (int32_t)(cur.w[0] & 15u) - 8));
    ed_shr8(cur);
  }
  return p;
}

// ---- [s]B + [h]P for PUBLIC s, h < L.  The per-lane table: entry j (0 .. 7) = (j + 1) P as ed_cached, 32 words; word w of entry j of lane `lane` of a
// batch of m lanes is the uint4 at table[(j * 8 + w / 4) * m + lane] -- neighbouring lanes read neighbouring 16-byte pieces.
constexpr size_t ED_TABLE_BYTES_PER_LANE = 8 * 128;
ECS_DEV void ed_table_store(uint4* __restrict__ table, size_t m, size_t lane, int j, const ed_cached& c) {
  const fe* f[4] = {&c.YpX, &c.YmX, &c.Z, &c.T2d};
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    table[((size_t)j * 8 + 2 * q) * m + lane] = make_uint4(f[q]->w[0], f[q]->w[1], f[q]->w[2], f[q]->w[3]);
    table[((size_t)j * 8 + 2 * q + 1) * m + lane] = make_uint4(f[q]->w[4], f[q]->w[5], f[q]->w[6], f[q]->w[7]);
  }
}
ECS_DEV ed_cached ed_table_load(const uint4* __restrict__ table, size_t m, size_t lane, uint32_t j) {
  ed_cached c;
  fe* f[4] = {&c.YpX, &c.YmX, &c.Z, &c.T2d};
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const uint4 lo = table[((size_t)j * 8 + 2 * q) * m + lane], hi = table[((size_t)j * 8 + 2 * q + 1) * m + lane];
    f[q]->w[0] = lo.x; f[q]->w[1] = lo.y; f[q]->w[2] = lo.z; f[q]->w[3] = lo.w;
    f[q]->w[4] = hi.x; f[q]->w[5] = hi.y; f[q]->w[6] = hi.z; f[q]->w[7] = hi.w;
  }
  return c;
}
// 1 .. 8 times p into the lane's table
ECS_DEV void ed_table_build(uint4* __restrict__ table, size_t m, size_t lane, const ed_point& p) {
  const ed_cached c1 = ed_to_cached(p);
  ed_table_store(table, m, lane, 0, c1);
  ed_point q = p;
#pragma unroll 1
  for (int j = 1; j < 8; ++j) {
    q = ed_add_cached(q, c1);
    ed_table_store(table, m, lane, j, ed_to_cached(q));
  }
}
ECS_DEV ed_point ed_straus_vartime(const fe& s, const fe& h, const uint4* __restrict__ table, size_t m, size_t lane) {
  fe bs = ed_digits_of(s), bh = ed_digits_of(h);
  ed_point p = ed_identity();
#pragma unroll 1
  for (int i = 63; i >= 0; --i) {
    p = ed_dbl4(p);
    const int32_t ds = (int32_t)(bs.w[7] >> 28) - 8, dh = (int32_t)(bh.w[7] >> 28) - 8;
    ed_shl4(bs); ed_shl4(bh);
    if (ds != 0) {
      const uint32_t mag = (uint32_t)(ds < 0 ? -ds : ds);
      const uint32_t* t = ED25519_BASE + (mag - 1) * 24;
      ed_precomp e;
#pragma unroll
      for (int q = 0; q < 8; ++q) { e.ypx.w[q] = t[q]; e.ymx.w[q] = t[8 + q]; e.xy2d.w[q] = t[16 + q]; }
      if (ds < 0) { const fe sw = e.ypx; e.ypx = e.ymx; e.ymx = sw; e.xy2d = fe25519_neg(e.xy2d); }
      p = ed_add_precomp(p, e);
    }
    if (dh != 0) {
      const uint32_t mag = (uint32_t)(dh < 0 ? -dh : dh);
      ed_cached c = ed_table_load(table, m, lane, mag - 1);
      if (dh < 0) { const fe sw = c.YpX; c.YpX = c.YmX; c.YmX = sw; c.T2d = fe25519_neg(c.T2d); }
      p = ed_add_cached(p, c);
    }
  }
  return p;
}

// ---- scalars modulo L (M = L's gmod).  Montgomery products take any 256-bit first operand: a b R^-1 + q L < 2 L before the one conditional subtraction.
// v mod L for any 256-bit v: v * (R mod L) * R^-1
ECS_DEV fe ed_sc_reduce256(const fe& v, const gmod& M) { return g_mul(v, g_words(M.r), M); }
// (hi 2^256 + lo) mod L: two Montgomery products, hi * R^2 * R^-1 + lo * R * R^-1
ECS_DEV fe ed_sc_reduce512(const fe& lo, const fe& hi, const gmod& M) { return g_add(g_mul(hi, g_words(M.rsq), M), ed_sc_reduce256(lo, M), M); }
// r + k a mod L (r, k < L; a any 256-bit value)
ECS_DEV fe ed_sc_muladd(const fe& r, const fe& k, const fe& a, const gmod& M) { return g_add(r, g_mul(g_mul(a, k, M), g_words(M.rsq), M), M); }
// all ones where s < L
ECS_DEV uint32_t ed_sc_below_L(const fe& s) { fe t; return sub8_3(t, s, fe25519_const<ed25519_consts::L>()); }

}  // namespace ecsimd_hip
