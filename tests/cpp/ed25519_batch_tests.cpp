// ed25519_batch_tests.cpp -- Ed25519 batch verification through the C++ host API (hip::ed25519_verify_batch, hip::ed25519_verify_cofactored,
// hip::ed25519_batch_randomizers, hip::ed25519_batch_plan, hip::ed25519_msm, hip::ed25519_msm_plan): a signed batch is accepted on every route, one forgery
// refuses it and the per-lane rule names it, a small-order lane is accepted by the equation and refused by the flag, the sum of [k]B terms, and the plans.
// Built and run by tests/test_cpp_ed25519_batch.py; the harness is mini_test.h.
#include <ecsimd/ecsimd.h>
#include <ecsimd/ed25519_batch.h>
#include "mini_test.h"

using namespace ecsimd;

namespace {
constexpr int ROUTES[] = {ECSIMD_ED25519_BATCH_MSM, ECSIMD_ED25519_BATCH_LANES, ECSIMD_ED25519_BATCH_AUTO};
using rows = std::vector<std::vector<uint8_t>>;

struct signed_batch {
  std::vector<uint8_t> records;
  hip::byte_records pk, sig;
  signed_batch(size_t n) : records(n * 45) {                                                   // 37-byte messages, 45 bytes apart
    rows seeds(n, std::vector<uint8_t>(32));
    for (size_t i = 0; i < n; ++i) for (size_t j = 0; j < 32; ++j) seeds[i][j] = (uint8_t)(i * 31 + j * 7 + (i >> 8));
    for (size_t i = 0; i < records.size(); ++i) records[i] = (uint8_t)(i * 131 + (i >> 8));
    const auto made = hip::ed25519_sign(hip::byte_records(seeds, 32), messages());
    sig = made.first; pk = made.second;
  }
  hip::messages messages() const { return hip::messages(records.data(), records.size() / 45, 37, 45); }
};
bool one(hip::mask const& m) { return m.size() == 1 && m.get(0); }
}  // namespace

TEST(Ed25519Batch, ASignedBatchIsAcceptedOnEveryRoute) {
  for (size_t n : {(size_t)1, (size_t)17, (size_t)300}) {
    const signed_batch b(n);
    EXPECT_TRUE(hip::ed25519_verify(b.pk, b.messages(), b.sig).count() == n);
    EXPECT_TRUE(hip::ed25519_verify_cofactored(b.pk, b.messages(), b.sig).count() == n);
    for (int route : ROUTES) {
      EXPECT_TRUE(one(hip::ed25519_verify_batch(b.pk, b.messages(), b.sig, nullptr, route)));
      EXPECT_TRUE(one(hip::ed25519_verify_batch(b.pk, b.messages(), b.sig, nullptr, route | ECSIMD_ED25519_REJECT_SMALL_ORDER)));
    }
    const rows z = hip::ed25519_batch_randomizers(b.pk, b.messages(), b.sig).host();
    EXPECT_TRUE(z.size() == n);
    for (auto const& r : z) {
      bool high = false;
      for (size_t j = 16; j < 32; ++j) high = high || r[j] != 0;
      EXPECT_TRUE((r[0] & 1) == 1 && !high);
    }
    EXPECT_TRUE(z == hip::ed25519_batch_randomizers(b.pk, b.messages(), b.sig).host());        // nothing is drawn
  }
  const std::vector<uint8_t> nothing;
  EXPECT_TRUE(one(hip::ed25519_verify_batch(hip::byte_records(0, 32), hip::messages(nothing.data(), 0, 0, 0), hip::byte_records(0, 64))));     // the empty batch
}

TEST(Ed25519Batch, OneForgeryRefusesTheBatchAndThePerLaneRuleNamesIt) {
  const size_t n = 300;
  signed_batch b(n);
  rows s = b.sig.host();
  s[123][40] ^= 4;
  const hip::byte_records forged(s, 64);
  const std::vector<uint8_t> lanes = hip::ed25519_verify_cofactored(b.pk, b.messages(), forged).host();
  for (size_t i = 0; i < n; ++i) EXPECT_TRUE(lanes[i] == (i == 123 ? 0 : 1));
  for (int route : ROUTES) EXPECT_TRUE(!hip::ed25519_verify_batch(b.pk, b.messages(), forged, nullptr, route).get(0));
  b.records[45 * 299 + 36] ^= 1;                                                               // the last byte of the last message
  for (int route : ROUTES) EXPECT_TRUE(!hip::ed25519_verify_batch(b.pk, b.messages(), b.sig, nullptr, route).get(0));
  b.records[45 * 299 + 36] ^= 1;
  for (int route : ROUTES) EXPECT_TRUE(one(hip::ed25519_verify_batch(b.pk, b.messages(), b.sig, nullptr, route)));
  int refused = 0;                                                                             // operands of different length are refused before the device sees them
  try { (void)hip::ed25519_verify_batch(hip::byte_records(n - 1, 32), b.messages(), b.sig); } catch (std::exception const&) { ++refused; }
  try { (void)hip::ed25519_verify_batch(b.pk, b.messages(), b.sig, nullptr, 6); } catch (hip::error const&) { ++refused; }         // and so is a flag that is no route
  EXPECT_EQ(refused, 2);
}

TEST(Ed25519Batch, ASmallOrderLaneIsAcceptedByTheEquationAndRefusedByTheFlag) {
  signed_batch b(17);
  rows pks = b.pk.host(), sigs = b.sig.host();
  pks[5] = std::vector<uint8_t>(32, 0); pks[5][0] = 1;                                         // A = the identity, R = the point of order 2, s = 0: 8 (-R) is the identity
  sigs[5] = std::vector<uint8_t>(64, 0);
  for (size_t j = 0; j < 32; ++j) sigs[5][j] = 0xff;
  sigs[5][0] = 0xec; sigs[5][31] = 0x7f;
  const hip::byte_records pk(pks, 32), sig(sigs, 64);
  EXPECT_TRUE(hip::ed25519_verify(pk, b.messages(), sig).get(5) == 0);                           // the cofactorless rule refuses it
  EXPECT_TRUE(hip::ed25519_verify_cofactored(pk, b.messages(), sig).count() == 17);
  EXPECT_TRUE(hip::ed25519_verify_cofactored(pk, b.messages(), sig, nullptr, true).count() == 16);
  for (int route : ROUTES) {
    EXPECT_TRUE(one(hip::ed25519_verify_batch(pk, b.messages(), sig, nullptr, route)));
    EXPECT_TRUE(!hip::ed25519_verify_batch(pk, b.messages(), sig, nullptr, route | ECSIMD_ED25519_REJECT_SMALL_ORDER).get(0));
  }
}

TEST(Ed25519Batch, TheSumOfTermsOnTheBasePoint) {
  // B's encoding 300 times under the scalars 1 .. 300 is [45150]B, which is also one term with that scalar; a refused encoding is counted
  const size_t n = 300;
  std::vector<uint8_t> B(32, 0x66); B[0] = 0x58;
  rows pts(n, B), ks(n, std::vector<uint8_t>(32, 0));
  for (size_t i = 0; i < n; ++i) { ks[i][0] = (uint8_t)(i + 1); ks[i][1] = (uint8_t)((i + 1) >> 8); }
  rows one_k(1, std::vector<uint8_t>(32, 0)); one_k[0][0] = (uint8_t)(45150 & 0xff); one_k[0][1] = (uint8_t)(45150 >> 8);
  const auto sum = hip::ed25519_msm(hip::byte_records(ks, 32), hip::byte_records(pts, 32));
  const auto single = hip::ed25519_msm(hip::byte_records(one_k, 32), hip::byte_records(rows(1, B), 32), 16);
  EXPECT_TRUE(sum.finite && sum.invalid == 0 && single.finite && sum.encoding == single.encoding && sum.encoding != B);
  pts[7] = std::vector<uint8_t>(32, 0); pts[7][0] = 2;                                         // y = 2 is on no point
  const auto without = hip::ed25519_msm(hip::byte_records(ks, 32), hip::byte_records(pts, 32));
  one_k[0][0] = (uint8_t)((45150 - 8) & 0xff); one_k[0][1] = (uint8_t)((45150 - 8) >> 8);
  EXPECT_TRUE(without.invalid == 1 && without.encoding == hip::ed25519_msm(hip::byte_records(one_k, 32), hip::byte_records(rows(1, B), 32)).encoding);
  const auto empty = hip::ed25519_msm(hip::byte_records(0, 32), hip::byte_records(0, 32));
  std::vector<uint8_t> identity(32, 0); identity[0] = 1;
  EXPECT_TRUE(!empty.finite && empty.invalid == 0 && empty.encoding == identity);
}

TEST(Ed25519Batch, ThePlansNeedNoDeviceAndRefuseWhatTheCallsRefuse) {
  const auto lanes = hip::ed25519_batch_plan(100, 32, ECSIMD_ED25519_BATCH_LANES), forced = hip::ed25519_batch_plan(100, 32, ECSIMD_ED25519_BATCH_MSM);
  EXPECT_TRUE(lanes.route == ECSIMD_ED25519_BATCH_LANES && lanes.launches == 3 && lanes.workspace_bytes > 0);
  const int msm = hip::ed25519_msm_plan(100, 128).launches + hip::ed25519_msm_plan(101, 253).launches;      // the two sums; two tree levels each
  EXPECT_TRUE(forced.route == ECSIMD_ED25519_BATCH_MSM && forced.launches == 5 + 2 + 2 + msm);
  EXPECT_TRUE(hip::ed25519_batch_plan(0, 32).launches == 1);
  const size_t top = ECSIMD_MSM_MAX_N - 1;
  EXPECT_TRUE(hip::ed25519_batch_plan(top, 32).route == (top >= ECSIMD_ED25519_BATCH_AUTO_THRESHOLD ? ECSIMD_ED25519_BATCH_MSM : ECSIMD_ED25519_BATCH_LANES));
  EXPECT_TRUE(hip::ed25519_batch_plan(100, 32).route == ECSIMD_ED25519_BATCH_LANES);
  const auto p = hip::ed25519_msm_plan(300, 253);
  EXPECT_TRUE(p.route == ECSIMD_MSM_ALG_BUCKETS && p.L == 8 && p.c * p.windows >= 253);
  int refused = 0;
  try { (void)hip::ed25519_batch_plan(ECSIMD_MSM_MAX_N, 32); } catch (hip::error const&) { ++refused; }
  try { (void)hip::ed25519_batch_plan(8, 32, 6); } catch (hip::error const&) { ++refused; }
  try { (void)hip::ed25519_msm_plan(8, 256, ECSIMD_MSM_ALG_LANES); } catch (hip::error const&) { ++refused; }
  try { (void)hip::ed25519_msm_plan(8, 257); } catch (hip::error const&) { ++refused; }
  EXPECT_EQ(refused, 4);
}

int main() { return mini::run_all(); }
