// bls12_381_tests.cpp -- BLS12-381 G1 through the C++ host API (hip::bls12_381::g1_*): the generator in both encodings, 2 G by g1_mul, the subgroup flags, a
// refused record through `ok`, and the two sums on both routes against g1_mul and g1_point_sum.  The expected bytes are the curve facts tools/bls12_381_model.py
// asserts.  Built and run by tests/test_cpp_bls12_381.py; the harness is mini_test.h.
#include <ecsimd/ecsimd.h>
#include <ecsimd/bls12_381.h>
#include "mini_test.h"

using namespace ecsimd;
using namespace ecsimd::literals;
namespace g1 = ecsimd::hip::bls12_381;

namespace {
template <size_t N> std::vector<uint8_t> vec(std::array<uint8_t, N> const& a) { return std::vector<uint8_t>(a.begin(), a.end()); }
std::vector<uint8_t> cat(std::vector<uint8_t> a, std::vector<uint8_t> const& b) { a.insert(a.end(), b.begin(), b.end()); return a; }
const auto GX = vec("17f1d3a73197d7942695638c4fa9ac0fc3688c4f9774b905a14e3a3f171bac586c55e83ff97a1aeffb3af00adb22c6bb"_hex);
const auto GY = vec("08b3f481e3aaa0f1a09e30ed741d8ae4fcf5e095d5d00af600db18cb2c04b3edd03cc744a2888ae40caa232946c5e7e1"_hex);
const auto X_2G = vec("0572cbea904d67468808c8eb50a9450c9721db309128012543902d0ac358a62ae28f75bb8f1c7c42c39a8c5529bf0f4e"_hex);
std::vector<uint8_t> scalar(uint64_t v) { std::vector<uint8_t> k(32, 0); for (int i = 0; i < 8; ++i) k[i] = (uint8_t)(v >> (8 * i)); return k; }
std::vector<uint8_t> infinity96() { std::vector<uint8_t> b(96, 0); b[0] = 0x40; return b; }
}  // namespace

TEST(Bls12381, TheGeneratorInBothEncodingsAndItsDouble) {
  const auto g = cat(GX, GY);
  auto gc = GX; gc[0] |= 0x80;                                  // y(G) is the smaller root: the compressed generator starts with 0x97
  EXPECT_TRUE(gc[0] == 0x97);
  std::vector<std::vector<uint8_t>> pts = {g, infinity96(), g};
  pts[2][95] ^= 1;                                              // off the curve
  const auto [c, ok] = g1::g1_compress(hip::byte_records(pts, 96));
  EXPECT_TRUE(ok.host() == (std::vector<uint8_t>{1, 1, 0}));
  EXPECT_TRUE(c.get(0) == gc && c.get(1)[0] == 0xc0 && c.get(2) == std::vector<uint8_t>(48, 0));
  const auto [u, ok2] = g1::g1_decompress(c);
  EXPECT_TRUE(ok2.host() == (std::vector<uint8_t>{1, 1, 0}) && u.get(0) == g && u.get(1) == infinity96());
  const auto [on, sub] = g1::g1_check(hip::byte_records(pts, 96));
  EXPECT_TRUE(on.host() == (std::vector<uint8_t>{1, 1, 0}) && sub.host() == on.host());
  const auto [twice, ok3] = g1::g1_mul(hip::byte_records({scalar(2), scalar(0), scalar(1)}, 32), hip::byte_records({g, g, g}, 96));
  EXPECT_TRUE(ok3.host() == std::vector<uint8_t>(3, 1));
  const auto two_g = twice.get(0);
  EXPECT_TRUE(std::vector<uint8_t>(two_g.begin(), two_g.begin() + 48) == X_2G && twice.get(1) == infinity96() && twice.get(2) == g);
}

TEST(Bls12381, BothRoutesOfTheSumAgreeWithTheLanes) {
  const size_t n = 67;                                          // a whole wave and a partial one
  const auto g = cat(GX, GY);
  std::vector<std::vector<uint8_t>> ks, pts(n, g);
  uint64_t total = 0;
  for (size_t i = 0; i < n; ++i) { ks.push_back(scalar(1000 * i + 7)); total += 1000 * i + 7; }
  pts[5][95] ^= 1;                                              // malformed: contributes nothing, counted
  total -= 1000 * 5 + 7;
  const hip::byte_records k(ks, 32), p(pts, 96);
  const auto want = g1::g1_mul(hip::byte_records({scalar(total)}, 32), hip::byte_records({g}, 96)).first.get(0);
  for (int alg : {ECSIMD_MSM_ALG_BUCKETS, ECSIMD_MSM_ALG_LANES, ECSIMD_MSM_ALG_AUTO}) {
    const auto r = g1::g1_msm(k, p, 64, alg);
    EXPECT_TRUE(r.encoding == want && r.finite && r.invalid == 1);
  }
  const auto s = g1::g1_point_sum(p);
  EXPECT_TRUE(s.encoding == g1::g1_mul(hip::byte_records({scalar(n - 1)}, 32), hip::byte_records({g}, 96)).first.get(0) && s.invalid == 1);
  const auto e = g1::g1_msm(hip::byte_records(0, 32), hip::byte_records(0, 96));
  EXPECT_TRUE(e.encoding == infinity96() && !e.finite && e.invalid == 0);
  const auto plan = g1::g1_msm_plan(n, 64, ECSIMD_MSM_ALG_BUCKETS);
  EXPECT_TRUE(plan.route == ECSIMD_MSM_ALG_BUCKETS && plan.windows * plan.c >= 64);
}

int main() { return mini::run_all(); }
