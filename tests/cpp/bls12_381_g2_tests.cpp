// bls12_381_g2_tests.cpp -- BLS12-381 G2 through the C++ host API (hip::bls12_381::g2_*): the generator in both encodings, 2 G2 by g2_mul, the subgroup flags, a
// refused record through `ok`, and the two sums on both routes against each other, g2_mul and g2_point_sum.  The expected bytes are the curve facts
// tools/bls12_381_g2_model.py asserts.  Built and run by tests/test_cpp_bls12_381_g2.py; the harness is mini_test.h.
#include <ecsimd/ecsimd.h>
#include <ecsimd/bls12_381_g2.h>
#include "mini_test.h"

using namespace ecsimd;
using namespace ecsimd::literals;
namespace g2 = ecsimd::hip::bls12_381;

namespace {
template <size_t N> std::vector<uint8_t> vec(std::array<uint8_t, N> const& a) { return std::vector<uint8_t>(a.begin(), a.end()); }
std::vector<uint8_t> cat(std::vector<uint8_t> a, std::vector<uint8_t> const& b) { a.insert(a.end(), b.begin(), b.end()); return a; }
const auto GX0 = vec("024aa2b2f08f0a91260805272dc51051c6e47ad4fa403b02b4510b647ae3d1770bac0326a805bbefd48056c8c121bdb8"_hex);
const auto GX1 = vec("13e02b6052719f607dacd3a088274f65596bd0d09920b61ab5da61bbdc7f5049334cf11213945d57e5ac7d055d042b7e"_hex);
const auto GY0 = vec("0ce5d527727d6e118cc9cdc6da2e351aadfd9baa8cbdd3a76d429a695160d12c923ac9cc3baca289e193548608b82801"_hex);
const auto GY1 = vec("0606c4a02ea734cc32acd2b02bc28b99cb3e287e85a763af267492ab572e99ab3f370d275cec1da1aaa9075ff05f79be"_hex);
std::vector<uint8_t> scalar(uint64_t v) { std::vector<uint8_t> k(32, 0); for (int i = 0; i < 8; ++i) k[i] = (uint8_t)(v >> (8 * i)); return k; }
std::vector<uint8_t> infinity192() { std::vector<uint8_t> b(192, 0); b[0] = 0x40; return b; }
std::vector<uint8_t> generator() { return cat(cat(GX1, GX0), cat(GY1, GY0)); }          // the wire order: c1 first
}  // namespace

TEST(Bls12381G2, TheGeneratorInBothEncodingsAndItsDouble) {
  const auto g = generator();
  auto gc = cat(GX1, GX0); gc[0] |= 0x80;                        // y(G2) is the smaller root: the compressed generator starts with 0x93
  EXPECT_TRUE(gc[0] == 0x93);
  std::vector<std::vector<uint8_t>> pts = {g, infinity192(), g};
  pts[2][191] ^= 1;                                             // off the curve
  const auto [c, ok] = g2::g2_compress(hip::byte_records(pts, 192));
  EXPECT_TRUE(ok.host() == (std::vector<uint8_t>{1, 1, 0}));
  EXPECT_TRUE(c.get(0) == gc && c.get(1)[0] == 0xc0 && c.get(2) == std::vector<uint8_t>(96, 0));
  const auto [u, ok2] = g2::g2_decompress(c);
  EXPECT_TRUE(ok2.host() == (std::vector<uint8_t>{1, 1, 0}) && u.get(0) == g && u.get(1) == infinity192() && u.get(2) == std::vector<uint8_t>(192, 0));
  const auto [on, sub] = g2::g2_check(hip::byte_records(pts, 192));
  EXPECT_TRUE(on.host() == (std::vector<uint8_t>{1, 1, 0}) && sub.host() == on.host());
  const auto [twice, ok3] = g2::g2_mul(hip::byte_records({scalar(2), scalar(0), scalar(1)}, 32), hip::byte_records({g, g, g}, 192));
  EXPECT_TRUE(ok3.host() == std::vector<uint8_t>(3, 1));
  EXPECT_TRUE(twice.get(1) == infinity192() && twice.get(2) == g);
  const auto sum = g2::g2_point_sum(hip::byte_records({g, g}, 192));                       // 2 G2 the other way: the sum of two equal points
  EXPECT_TRUE(sum.encoding == twice.get(0) && sum.finite && sum.invalid == 0 && twice.get(0) != g);
  const auto [on2, sub2] = g2::g2_check(hip::byte_records({twice.get(0)}, 192));
  EXPECT_TRUE(on2.host() == std::vector<uint8_t>{1} && sub2.host() == std::vector<uint8_t>{1});
}

TEST(Bls12381G2, BothRoutesOfTheSumAgreeWithTheLanes) {
  const size_t n = 67;                                          // a whole wave and a partial one
  const auto g = generator();
  std::vector<std::vector<uint8_t>> ks, pts(n, g);
  uint64_t total = 0;
  for (size_t i = 0; i < n; ++i) { ks.push_back(scalar(1000 * i + 7)); total += 1000 * i + 7; }
  pts[5][191] ^= 1;                                             // malformed: contributes nothing, counted
  total -= 1000 * 5 + 7;
  const hip::byte_records k(ks, 32), p(pts, 192);
  const auto want = g2::g2_mul(hip::byte_records({scalar(total)}, 32), hip::byte_records({g}, 192)).first.get(0);
  for (int alg : {ECSIMD_MSM_ALG_BUCKETS, ECSIMD_MSM_ALG_LANES, ECSIMD_MSM_ALG_AUTO}) {
    const auto r = g2::g2_msm(k, p, 64, alg);
    EXPECT_TRUE(r.encoding == want && r.finite && r.invalid == 1);
  }
  const auto s = g2::g2_point_sum(p);
  EXPECT_TRUE(s.encoding == g2::g2_mul(hip::byte_records({scalar(n - 1)}, 32), hip::byte_records({g}, 192)).first.get(0) && s.invalid == 1);
  const auto sc = g2::g2_point_sum(g2::g2_compress(p).first);                              // the compressed form: the refused lane is 96 zero bytes, malformed again
  EXPECT_TRUE(sc.encoding == s.encoding && sc.invalid == 1);
  const auto e = g2::g2_msm(hip::byte_records(0, 32), hip::byte_records(0, 192));
  EXPECT_TRUE(e.encoding == infinity192() && !e.finite && e.invalid == 0);
  const auto plan = g2::g2_msm_plan(n, 64, ECSIMD_MSM_ALG_BUCKETS);
  EXPECT_TRUE(plan.route == ECSIMD_MSM_ALG_BUCKETS && plan.windows * plan.c >= 64);
}

int main() { return mini::run_all(); }
