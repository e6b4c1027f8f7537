// schnorr_batch_tests.cpp -- BIP-340 batch verification through the C++ host API (curve_group<curve_secp256k1>::schnorr_verify_batch, hip::schnorr_verify_batch,
// hip::schnorr_batch_plan): a signed batch is accepted on every route, one forgery refuses it, and the plan.  Built and run by tests/test_cpp_schnorr_batch.py;
// the harness is mini_test.h.
#include <ecsimd/ecsimd.h>
#include <ecsimd/schnorr_batch.h>
#include <ecsimd/msm.h>
#include "mini_test.h"

using namespace ecsimd;

namespace {
using W256 = wide_bignum<bignum_256>;
using CG = curve_group<curve_secp256k1>;
// the member exists for secp256k1 only, as schnorr_verify does
template <class G> concept has_batch = requires(W256 const& a, hip::messages const& m) { G::schnorr_verify_batch(a, m, a, a); };
static_assert(has_batch<curve_group<curve_secp256k1>> && !has_batch<curve_group<curve_nist_p256>>);
constexpr int ROUTES[] = {ECSIMD_SCHNORR_BATCH_MSM, ECSIMD_SCHNORR_BATCH_LANES, ECSIMD_SCHNORR_BATCH_AUTO};

struct signed_batch {
  std::vector<uint8_t> records;
  W256 px, r, s;
  signed_batch(size_t n) : records(n * 45) {                                                   // 37-byte messages, 45 bytes apart
    const W256 d(n, [](size_t i, size_t) { bignum_256 b; b.limbs = {0x9e3779b97f4a7c15ull * (i + 1), i * 77, ~i, 0x0123456789abcdefull ^ (i << 20)}; return b; });
    for (size_t i = 0; i < records.size(); ++i) records[i] = (uint8_t)(i * 131 + (i >> 8));
    hip::mask ok;
    const auto sig = CG::schnorr_sign(d, messages(), px, ok);
    EXPECT_TRUE(all(ok));
    r = sig.first; s = sig.second;
  }
  hip::messages messages() const { return hip::messages(records.data(), records.size() / 45, 37, 45); }
};
}  // namespace

TEST(SchnorrBatch, ASignedBatchIsAcceptedOnEveryRoute) {
  for (size_t n : {(size_t)1, (size_t)17, (size_t)300}) {
    const signed_batch b(n);
    EXPECT_TRUE(all(CG::schnorr_verify(b.px, b.messages(), b.r, b.s)));
    for (int route : ROUTES) {
      EXPECT_TRUE(CG::schnorr_verify_batch(b.px, b.messages(), b.r, b.s, route));
      const hip::mask on_device = hip::schnorr_verify_batch(b.px, b.messages(), b.r, b.s, route);
      EXPECT_TRUE(on_device.size() == 1 && on_device.get(0));
    }
  }
  const W256 none(0, bignum_256{});
  const std::vector<uint8_t> nothing;
  EXPECT_TRUE(CG::schnorr_verify_batch(none, hip::messages(nothing.data(), 0, 0, 0), none, none));     // the empty batch
}

TEST(SchnorrBatch, OneForgeryRefusesTheBatch) {
  const size_t n = 300;
  signed_batch b(n);
  std::vector<bignum_256> s = b.s.host();
  s[123].limbs[1] ^= 4;
  const W256 forged(s);
  EXPECT_TRUE(!CG::schnorr_verify(b.px, b.messages(), b.r, forged).get(123));
  for (int route : ROUTES) EXPECT_TRUE(!CG::schnorr_verify_batch(b.px, b.messages(), b.r, forged, route));
  b.records[45 * 299 + 36] ^= 1;                                                               // the last byte of the last message
  for (int route : ROUTES) EXPECT_TRUE(!CG::schnorr_verify_batch(b.px, b.messages(), b.r, b.s, route));
  b.records[45 * 299 + 36] ^= 1;
  for (int route : ROUTES) EXPECT_TRUE(CG::schnorr_verify_batch(b.px, b.messages(), b.r, b.s, route));
  bool refused = false;                                                                        // operands of different length are refused before the device sees them
  try { (void)CG::schnorr_verify_batch(W256(n - 1, bignum_256::from(5)), b.messages(), b.r, b.s); } catch (std::exception const&) { refused = true; }
  EXPECT_TRUE(refused);
  refused = false;                                                                             // and so is a flag that is no route
  try { (void)CG::schnorr_verify_batch(b.px, b.messages(), b.r, b.s, 3); } catch (hip::error const&) { refused = true; }
  EXPECT_TRUE(refused);
}

TEST(SchnorrBatch, ThePlanNeedsNoDeviceAndRefusesWhatTheCallRefuses) {
  const auto small = hip::schnorr_batch_plan(100, 32), forced = hip::schnorr_batch_plan(100, 32, ECSIMD_SCHNORR_BATCH_MSM);
  EXPECT_TRUE(small.route == ECSIMD_SCHNORR_BATCH_LANES && small.launches == 10 && small.workspace_bytes > 0);
  const int msm = hip::msm_plan(100, 128, ECSIMD_MSM_ALG_BUCKETS).launches + hip::msm_plan(101, 256, ECSIMD_MSM_ALG_BUCKETS).launches;   // the two sums; two tree levels each
  EXPECT_TRUE(forced.route == ECSIMD_SCHNORR_BATCH_MSM && forced.launches == 5 + 2 + 2 + msm);
  EXPECT_TRUE(hip::schnorr_batch_plan(0, 32).launches == 1);
  const size_t top = ECSIMD_MSM_MAX_N - 1;
  EXPECT_TRUE(hip::schnorr_batch_plan(top, 32).route == (top >= ECSIMD_SCHNORR_BATCH_AUTO_THRESHOLD ? ECSIMD_SCHNORR_BATCH_MSM : ECSIMD_SCHNORR_BATCH_LANES));
  int refused = 0;
  try { (void)hip::schnorr_batch_plan(ECSIMD_MSM_MAX_N, 32); } catch (hip::error const&) { ++refused; }
  try { (void)hip::schnorr_batch_plan(8, 32, 4); } catch (hip::error const&) { ++refused; }
  EXPECT_EQ(refused, 2);
}

int main() { return mini::run_all(); }
