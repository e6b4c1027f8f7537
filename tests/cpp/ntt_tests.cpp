// ntt_tests.cpp -- the number-theoretic transform through the C++ host API (hip::ntt::domain, forward, inverse, bitrev, plan): a delta and a constant have
// closed-form transforms, inverse undoes forward on a subgroup and on a coset at one and at several passes, a polynomial product against the schoolbook one in
// small integers, the bit reversal.  Built and run by tests/test_cpp_ntt.py; the harness is mini_test.h.
#include <ecsimd/ecsimd.h>
#include <ecsimd/ntt.h>
#include "mini_test.h"

using namespace ecsimd;
namespace ntt = ecsimd::hip::ntt;

namespace {
using W256 = wide_bignum<bignum_256>;
}

TEST(Ntt, PlanAndFieldFactsNeedNoDevice) {
  const auto fr = ntt::bls12_381_fr();
  EXPECT_EQ(ntt::info(fr.first).two_adicity, 32);
  EXPECT_TRUE(ntt::info(fr.first).root != fr.second);                      // the default rule starts from 5, the conventional root from 7
  EXPECT_EQ(ntt::info(ECSIMD_HIP_FIELD_P256_ORDER).two_adicity, 4);
  EXPECT_EQ(ntt::plan(9).passes, 1);
  EXPECT_EQ(ntt::plan(10).passes, 2);
  EXPECT_EQ(ntt::plan(6, 1, ECSIMD_NTT_MAX_RADIX_LOG(2)).passes, 3);
  EXPECT_TRUE(ntt::plan(9).workspace_bytes == 0 && ntt::plan(12, 3).workspace_bytes == (size_t)3 * 4096 * 32);
  bool threw = false;
  try { (void)ntt::plan(25); } catch (hip::error const&) { threw = true; }
  EXPECT_TRUE(threw);
}

TEST(Ntt, ClosedFormsRoundTripsAndAProduct) {
  const auto fr = ntt::bls12_381_fr();
  const bignum_256 seven = bignum_256::from(7);
  for (int log_n : {1, 4, 9, 11}) {
    const size_t n = (size_t)1 << log_n;
    const ntt::domain H(fr.first, log_n, &fr.second), C(fr.first, log_n, &fr.second, &seven);
    // a delta at 0 transforms to the constant; a constant c to n c at 0 and 0 elsewhere
    const W256 delta(n, [](size_t i, size_t) { return bignum_256::from(i == 0 ? 5 : 0); });
    const auto fd = ntt::forward(H, delta).host();
    bool all5 = true;
    for (auto const& v : fd) all5 = all5 && v == bignum_256::from(5);
    EXPECT_TRUE(all5);
    const auto fc = ntt::forward(H, W256(n, bignum_256::from(3))).host();
    bool shape = fc[0] == bignum_256::from(3 * n);
    for (size_t i = 1; i < n; ++i) shape = shape && fc[i] == bignum_256::from(0);
    EXPECT_TRUE(shape);
    // two arrays at once, every schedule the hook reaches: inverse(forward(x)) == x
    const W256 x(2 * n, [](size_t i, size_t) { bignum_256 v; v.limbs = {i * 0x9e3779b97f4a7c15ull + 1, ~i, i * i, i & 0xffff}; return v; });
    for (int flags : {0, ECSIMD_NTT_MAX_RADIX_LOG(1), ECSIMD_NTT_MAX_RADIX_LOG(3)})
      for (ntt::domain const* d : {&H, &C}) EXPECT_TRUE(ntt::inverse(*d, ntt::forward(*d, x, flags), flags).host() == x.host());
    EXPECT_TRUE(ntt::bitrev(log_n, ntt::bitrev(log_n, x)).host() == x.host());
  }
  // (1 + 2 x + 3 x^2)(4 + 5 x) = 4 + 13 x + 22 x^2 + 15 x^3 on a domain of 8
  const ntt::domain H(fr.first, 3, &fr.second);
  const uint64_t a[8] = {1, 2, 3}, b[8] = {4, 5}, want[8] = {4, 13, 22, 15};
  const W256 A(8, [&](size_t i, size_t) { return bignum_256::from(a[i]); }), B(8, [&](size_t i, size_t) { return bignum_256::from(b[i]); });
  const W256 fa = ntt::forward(H, A), fb = ntt::forward(H, B), prod = W256::uninitialized(8);
  hip::check(ecsimd_hip_mod_mul(hip::context(), fr.first, fa.data(), fb.data(), prod.data(), 8), "ecsimd_hip_mod_mul");
  const auto got = ntt::inverse(H, prod).host();
  for (size_t i = 0; i < 8; ++i) EXPECT_TRUE(got[i] == bignum_256::from(want[i]));
  const auto r = ntt::bitrev(3, A).host();
  EXPECT_TRUE(r[0] == bignum_256::from(1) && r[4] == bignum_256::from(2) && r[2] == bignum_256::from(3));
}

int main() { return mini::run_all(); }
