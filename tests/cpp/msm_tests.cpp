// msm_tests.cpp -- multi-scalar multiplication through the C++ host API (hip::msm<Curve>, hip::point_sum<Curve>, hip::msm_plan): the three routes against the
// per-lane products summed by the group law the API already has, cancelling terms, an invalid point, and the plan.  Built and run by tests/test_cpp_msm.py;
// the harness is mini_test.h.
#include <ecsimd/ecsimd.h>
#include <ecsimd/msm.h>
#include "mini_test.h"

using namespace ecsimd;

namespace {
using W256 = wide_bignum<bignum_256>;
template <class Curve> struct scenario {
  using CG = curve_group<Curve>;
  using WCP = wide_curve_point<Curve>;
  // P_i = (i + 1) G and k_i: then sum k_i P_i = (sum k_i (i + 1)) G with small k_i, one scalar_mult_base
  static void run(size_t n) {
    const W256 a(n, [](size_t i, size_t) { return bignum_256::from(i + 1); });
    const WCP P = CG::scalar_mult_base_affine(a);
    const W256 k(n, [](size_t i, size_t) { return bignum_256::from(1000003 * (i + 7)); });
    unsigned __int128 total = 0, plain = 0;
    for (size_t i = 0; i < n; ++i) { total += (unsigned __int128)(1000003 * (i + 7)) * (i + 1); plain += i + 1; }
    bignum_256 t; t.limbs = {(uint64_t)total, (uint64_t)(total >> 64), 0, 0};
    const WCP want = CG::scalar_mult_base_affine(W256(1, t));
    for (int alg : {ECSIMD_MSM_ALG_BUCKETS, ECSIMD_MSM_ALG_LANES, ECSIMD_MSM_ALG_AUTO}) {
      const auto r = hip::msm<Curve>(k, P, 256, alg);
      EXPECT_TRUE(r.finite() && r.invalid == 0);
      EXPECT_TRUE(r.point->first == want.x().get(0) && r.point->second == want.y().get(0));
      const auto r64 = hip::msm<Curve>(k, P, 64, alg);                 // the scalars are below 2^64: the same sum from a quarter of the windows
      EXPECT_TRUE(r64.finite() && r64.point->first == want.x().get(0) && r64.point->second == want.y().get(0));
    }
    bignum_256 s; s.limbs = {(uint64_t)plain, 0, 0, 0};
    const WCP sum = CG::scalar_mult_base_affine(W256(1, s));
    const auto ps = hip::point_sum<Curve>(P);
    EXPECT_TRUE(ps.finite() && ps.invalid == 0 && ps.point->first == sum.x().get(0) && ps.point->second == sum.y().get(0));
  }
};
}  // namespace

TEST(Msm, AllRoutesGiveTheSumOnBothCurves) {
  for (size_t n : {(size_t)1, (size_t)65, (size_t)1500}) {
    scenario<curve_nist_p256>::run(n);
    scenario<curve_secp256k1>::run(n);
  }
}

TEST(Msm, EmptyCancellingAndInvalidBatches) {
  using CG = curve_group<curve_secp256k1>;
  using WCP = wide_curve_point<curve_secp256k1>;
  const auto none = hip::msm<curve_secp256k1>(W256(0, bignum_256{}), WCP{W256(0, bignum_256{}), W256(0, bignum_256{})});
  EXPECT_TRUE(!none.finite() && none.invalid == 0);
  // k G + k (-G) = infinity
  const WCP g2 = CG::scalar_mult_base_affine(W256(2, bignum_256::from(1)));
  std::vector<bignum_256> ys = g2.y().host();
  const bignum_256 p = CG::curve_constant(0);
  unsigned __int128 bw = 0;
  for (int i = 0; i < 4; ++i) { const unsigned __int128 d = (unsigned __int128)p.limbs[i] - ys[1].limbs[i] - (uint64_t)bw; ys[1].limbs[i] = (uint64_t)d; bw = (d >> 64) & 1; }
  const WCP pair{g2.x(), W256(ys)};                                      // G and -G
  for (int alg : {ECSIMD_MSM_ALG_BUCKETS, ECSIMD_MSM_ALG_LANES}) {
    const auto r = hip::msm<curve_secp256k1>(W256(2, bignum_256::from(12345)), pair, 256, alg);
    EXPECT_TRUE(!r.finite() && r.invalid == 0);
  }
  EXPECT_TRUE(!hip::point_sum<curve_secp256k1>(pair).finite());
  ys[1].limbs[0] ^= 1;                                                   // off the curve: left out and counted
  const WCP dirty{g2.x(), W256(ys)};
  const auto r = hip::msm<curve_secp256k1>(W256(2, bignum_256::from(1)), dirty);
  EXPECT_TRUE(r.finite() && r.invalid == 1 && r.point->first == g2.x().get(0) && r.point->second == g2.y().get(0));
  const auto ps = hip::point_sum<curve_secp256k1>(dirty);
  EXPECT_TRUE(ps.finite() && ps.invalid == 1 && ps.point->first == g2.x().get(0));
}

TEST(Msm, ThePlanNeedsNoDeviceAndRefusesWhatTheCallRefuses) {
  const auto p = hip::msm_plan((size_t)1 << 20);
  EXPECT_TRUE(p.route == ECSIMD_MSM_ALG_BUCKETS && p.c == 16 && p.windows == 16 && p.buckets == 65536u && p.L * p.L <= 4u << 20 && p.max_chain < 5000u);
  EXPECT_TRUE(hip::msm_plan(100).route == ECSIMD_MSM_ALG_LANES && hip::msm_plan(100, 256, ECSIMD_MSM_ALG_BUCKETS).route == ECSIMD_MSM_ALG_BUCKETS);
  int refused = 0;
  try { (void)hip::msm_plan(8, 0); } catch (hip::error const&) { ++refused; }
  try { (void)hip::msm_plan(((size_t)1 << 24) + 1); } catch (hip::error const&) { ++refused; }
  try { (void)hip::msm_plan(8, 256, 4); } catch (hip::error const&) { ++refused; }
  EXPECT_EQ(refused, 3);
}

int main() { return mini::run_all(); }
