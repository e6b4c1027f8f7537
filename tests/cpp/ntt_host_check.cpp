// ntt_host_check.cpp -- the number-theoretic transform's pass body (ecsimd_amd/csrc/ntt.cuh) on a CPU: every pass of every schedule, tile by tile and lane by
// lane, over ntt.cuh's portable field, against transforms computed by tools/ntt_model.py.  A stand-alone program: no GPU, no library; build it with
// -fsanitize=address,undefined to have every index of the pass body checked against the buffers' bounds.
//
//   ntt_host_check CASES     CASES: "field P ROOT S" (hex, hex, the two-adicity), then any number of
//                                   "case LOG_N SHIFT BATCH" followed by BATCH * 2^LOG_N inputs and as many forward outputs, one hex number per line.
// Every case runs forward and inverse at the default schedule and at ECSIMD_NTT_MAX_RADIX_LOG(1 .. 9), in place (the first pass of several then reads `out`
// and writes the workspace) and, at the default schedule, out of place.  The LDS image is poisoned before every tile, so a slot read before it is written shows.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../ecsimd_amd/csrc/ntt.cuh"

using namespace ecsimd_hip::ntt;

namespace {
struct u256 { uint32_t w[8]; };
u256 parse_hex(const std::string& s) {
  u256 r; memset(&r, 0, sizeof r);
  size_t start = (s.size() > 1 && s[0] == '0' && (s[1] == 'x' || s[1] == 'X')) ? 2 : 0;
  int nib = 0;
  for (size_t i = s.size(); i > start && nib < 64; --i, ++nib) {
    const char c = s[i - 1];
    const uint32_t v = c >= '0' && c <= '9' ? (uint32_t)(c - '0') : c >= 'a' && c <= 'f' ? (uint32_t)(c - 'a' + 10) : (uint32_t)(c - 'A' + 10);
    r.w[nib / 8] |= v << (4 * (nib % 8));
  }
  return r;
}
pel as_pel(const u256& v) { pel r; memcpy(r.w, v.w, sizeof r.w); return r; }
bool geq(const uint32_t* a, const uint32_t* b) { for (int i = 7; i >= 0; --i) if (a[i] != b[i]) return a[i] > b[i]; return true; }
void dbl_mod(uint32_t* a, const uint32_t* p) {
  const uint32_t top = a[7] >> 31;
  for (int i = 7; i > 0; --i) a[i] = (a[i] << 1) | (a[i - 1] >> 31);
  a[0] <<= 1;
  if (top || geq(a, p)) { uint64_t bw = 0; for (int i = 0; i < 8; ++i) { const uint64_t x = (uint64_t)a[i] - p[i] - bw; a[i] = (uint32_t)x; bw = (x >> 32) & 1u; } }
}
struct field { pfield F; pel one; u256 p; };
field make_field(const u256& p) {
  field K; K.p = p;
  memcpy(K.F.p, p.w, sizeof p.w);
  uint32_t t[8] = {1, 0, 0, 0, 0, 0, 0, 0};
  for (int i = 0; i < 256; ++i) dbl_mod(t, p.w);
  memcpy(K.one.w, t, sizeof t);                                  // R mod p
  for (int i = 0; i < 256; ++i) dbl_mod(t, p.w);
  memcpy(K.F.r2, t, sizeof t);                                   // R^2 mod p
  uint32_t inv = p.w[0];
  for (int i = 0; i < 5; ++i) inv *= 2u - p.w[0] * inv;
  K.F.mprime = 0u - inv;
  return K;
}
pel pow_pm2(const field& K, pel base) {                          // base^(p - 2), Montgomery form
  uint32_t e[8]; memcpy(e, K.p.w, sizeof e);
  for (uint64_t i = 0, bw = 2; i < 8; ++i) { const uint64_t x = (uint64_t)e[i] - bw; e[i] = (uint32_t)x; bw = (x >> 32) & 1u; }
  pel r = K.one;
  for (int i = 0; i < 256; ++i) { if ((e[i >> 5] >> (i & 31)) & 1u) r = K.F.mul(r, base); base = K.F.mul(base, base); }
  return r;
}
struct domain { int log_n, coset; std::vector<u4> block; size_t off[2][5]; };
domain make_domain(const field& K, const pel& root_m, int s, int log_n, const pel& g_m) {
  const pfield& F = K.F;
  domain D; D.log_n = log_n; D.coset = memcmp(g_m.w, K.one.w, sizeof g_m.w) != 0;
  pel w = root_m;
  for (int i = 0; i < s - log_n; ++i) w = F.mul(w, w);
  pel nm = K.one;
  for (int i = 0; i < log_n; ++i) nm = F.add(nm, nm);
  const pel ninv = pow_pm2(K, nm);
  const size_t n = (size_t)1 << log_n, lo_n = n < (size_t)SPLIT ? n : (size_t)SPLIT, hi_n = n > (size_t)SPLIT ? n >> SPLIT_LOG : 1;
  const int log_rt = log_n < DEFAULT_RADIX_LOG ? log_n : DEFAULT_RADIX_LOG;
  auto powers = [&](const pel& base, size_t count, pel t) { for (size_t i = 0; i < count; ++i) { u4 a, b; pfield::store(t, &a, &b); D.block.push_back(a); D.block.push_back(b); t = F.mul(t, base); } };
  auto pow2k = [&](pel v, int k) { for (int i = 0; i < k; ++i) v = F.mul(v, v); return v; };
  for (int dir = 0; dir < 2; ++dir) {
    const pel wd = dir ? pow_pm2(K, w) : w, gd = dir ? pow_pm2(K, g_m) : g_m;
    D.off[dir][0] = D.block.size(); powers(pow2k(wd, log_n - log_rt), (size_t)1 << (log_rt - 1), K.one);
    D.off[dir][1] = D.block.size(); powers(wd, lo_n, K.one);
    D.off[dir][2] = D.block.size(); powers(pow2k(wd, SPLIT_LOG), hi_n, K.one);
    D.off[dir][3] = D.block.size(); powers(gd, lo_n, K.one);
    D.off[dir][4] = D.block.size(); powers(pow2k(gd, SPLIT_LOG), hi_n, dir ? F.mul(ninv, pfield::one()) : F.mul(K.one, F.rsq()));
  }
  return D;
}
// One transform call as capi.hip enqueues it: the passes in order, each over all its tiles, each phase for every lane before the next.
void transform(const field& K, const domain& D, const std::vector<u4>& in_if_apart, std::vector<u4>& out, size_t batch, int cap, int inverse, bool in_place) {
  schedule S;
  if (!make_schedule(D.log_n, cap, &S)) { fprintf(stderr, "no schedule\n"); exit(2); }
  std::vector<u4> workspace(S.passes > 1 ? out.size() : 0), lds(LDS_SLOTS);
  const u4* src = in_place ? out.data() : in_if_apart.data();
  for (int i = 0; i < S.passes; ++i) {
    pass_args A;
    A.G = make_geom(D.log_n, S, i, batch, inverse, D.coset);
    const u4* b = D.block.data();
    A.tw = tables{b + D.off[inverse][0], b + D.off[inverse][1], b + D.off[inverse][2], b + D.off[inverse][3], b + D.off[inverse][4]};
    A.src = src;
    A.dst = pass_writes_workspace(i, S.passes) ? workspace.data() : out.data();
    if (A.src == A.dst && !A.G.last) { fprintf(stderr, "a pass that is not the last runs in place\n"); exit(2); }
    // a pass that runs in place may only do so because every tile writes the places it read: run the tiles in an order that would show otherwise
    const uint64_t tiles = tiles_of(A.G);
    for (uint64_t k = 0; k < tiles; ++k) {
      const uint64_t tile = tiles - 1 - k;
      memset(lds.data(), 0xA5, lds.size() * sizeof(u4));
      for (int lane = 0; lane < LANES; ++lane) pass_load(K.F, A, tile, lane, lds.data());
      for (int u = 0; u < A.G.log_r; ++u) for (int lane = LANES - 1; lane >= 0; --lane) pass_stage(K.F, A, tile, lane, u, lds.data());
      for (int lane = 0; lane < LANES; ++lane) pass_store(K.F, A, tile, lane, lds.data());
    }
    src = A.dst;
  }
}
std::vector<u4> pack(const std::vector<u256>& v) {
  std::vector<u4> r(2 * v.size());
  for (size_t i = 0; i < v.size(); ++i) { memcpy(r[2 * i].v, v[i].w, 16); memcpy(r[2 * i + 1].v, v[i].w + 4, 16); }
  return r;
}
u256 reduced(const field& K, const u256& v) { u256 r = v; while (geq(r.w, K.p.w)) { uint64_t bw = 0; for (int i = 0; i < 8; ++i) { const uint64_t x = (uint64_t)r.w[i] - K.p.w[i] - bw; r.w[i] = (uint32_t)x; bw = (x >> 32) & 1u; } } return r; }
size_t mismatches(const std::vector<u4>& got, const std::vector<u4>& want) {
  size_t bad = 0;
  for (size_t i = 0; i < want.size(); ++i) bad += memcmp(got[i].v, want[i].v, 16) != 0;
  return bad;
}
}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: ntt_host_check CASES\n"); return 2; }
  FILE* f = fopen(argv[1], "r");
  if (!f) { perror(argv[1]); return 2; }
  char a[160], b[160], c[160];
  int s = 0;
  if (fscanf(f, " field %150s %150s %d", a, b, &s) != 3) { fprintf(stderr, "no field line\n"); return 2; }
  const field K = make_field(parse_hex(a));
  const pel root_m = K.F.mul(as_pel(parse_hex(b)), K.F.rsq());
  size_t cases = 0, runs = 0, failures = 0;
  int log_n; unsigned long batch;
  while (fscanf(f, " case %d %150s %lu", &log_n, c, &batch) == 3) {
    const size_t total = (size_t)batch << log_n;
    std::vector<u256> in(total), fwd(total), in_mod(total);
    for (size_t i = 0; i < total; ++i) { if (fscanf(f, " %150s", a) != 1) return 2; in[i] = parse_hex(a); in_mod[i] = reduced(K, in[i]); }
    for (size_t i = 0; i < total; ++i) { if (fscanf(f, " %150s", a) != 1) return 2; fwd[i] = parse_hex(a); }
    const domain D = make_domain(K, root_m, s, log_n, K.F.mul(as_pel(parse_hex(c)), K.F.rsq()));
    const std::vector<u4> pin = pack(in), pfwd = pack(fwd), pmod = pack(in_mod);
    ++cases;
    for (int cap = DEFAULT_RADIX_LOG; cap >= 1; --cap) {
      for (int apart = 0; apart <= (cap == DEFAULT_RADIX_LOG ? 1 : 0); ++apart) {
        std::vector<u4> out = apart ? std::vector<u4>(pin.size()) : pin;
        transform(K, D, pin, out, batch, cap, 0, !apart);
        size_t bad = mismatches(out, pfwd);
        if (bad) { ++failures; printf("FAIL forward log_n %d shift %s batch %lu cap %d %s: %zu halves differ\n", log_n, c, batch, cap, apart ? "out of place" : "in place", bad); }
        out = apart ? std::vector<u4>(pin.size()) : pfwd;
        transform(K, D, pfwd, out, batch, cap, 1, !apart);
        bad = mismatches(out, pmod);
        if (bad) { ++failures; printf("FAIL inverse log_n %d shift %s batch %lu cap %d %s: %zu halves differ\n", log_n, c, batch, cap, apart ? "out of place" : "in place", bad); }
        runs += 2;
      }
    }
  }
  fclose(f);
  printf("%zu cases, %zu transforms, %zu failures\n", cases, runs, failures);
  return failures || !cases ? 1 : 0;
}
