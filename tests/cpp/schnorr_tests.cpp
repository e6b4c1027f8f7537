// schnorr_tests.cpp -- BIP-340 through the C++ host API (curve_group<curve_secp256k1>::schnorr_sign / schnorr_verify): the known answer, a round trip over
// strided messages, and what a changed message or key does.  Built and run by tests/test_cpp_schnorr.py on the GPU box; the harness is mini_test.h.
#include <ecsimd/ecsimd.h>
#include "mini_test.h"

using namespace ecsimd;
using namespace ecsimd::literals;

namespace {
using W256 = wide_bignum<bignum_256>;
using CG = curve_group<curve_secp256k1>;
template <size_t N> bignum_256 bn(std::array<uint8_t, N> const& be) { return bn_from_bytes_BE<bignum_256>(be); }
// the two members exist for secp256k1 only
template <class G> concept has_schnorr = requires(W256 const& a, hip::messages const& m) { G::schnorr_verify(a, m, a, a); };
static_assert(has_schnorr<curve_group<curve_secp256k1>> && !has_schnorr<curve_group<curve_nist_p256>>);
}  // namespace

TEST(Schnorr, Bip340VectorZero) {
  // secret key 3, aux and message 32 zero bytes
  const std::vector<std::string> zero(default_lanes, std::string(32, '\0'));
  const hip::messages m(zero);
  const W256 d{bignum_256::from(3)}, aux{bignum_256{}};
  W256 px; hip::mask ok;
  const auto sig = CG::schnorr_sign(d, m, px, ok, &aux);
  EXPECT_TRUE(all(ok));
  EXPECT_TRUE(px.get(0) == bn("F9308A019258C31049344F85F89D5229B531C845836F99B08601F113BCE036F9"_hex));
  EXPECT_TRUE(sig.first.get(0) == bn("E907831F80848D1069A5371B402410364BDF1C5F8307B0084C55F1CE2DCA8215"_hex));
  EXPECT_TRUE(sig.second.get(0) == bn("25F66A4A85EA8B71E482A74F382D2CE5EBEEE8FDB2172F477DF4900D310536C0"_hex));
  EXPECT_TRUE(all(CG::schnorr_verify(px, m, sig.first, sig.second)));
  // no aux = 32 zero bytes
  W256 px2; hip::mask ok2;
  const auto sig2 = CG::schnorr_sign(d, m, px2, ok2);
  EXPECT_TRUE(all(ok2) && all(sig2.first == sig.first) && all(sig2.second == sig.second) && all(px2 == px));
}

TEST(Schnorr, RoundTripOverARecordArray) {
  const size_t n = 300;
  const W256 d(n, [](size_t i, size_t) { bignum_256 b; b.limbs = {0x9e3779b97f4a7c15ull * (i + 1), i * 77, ~i, 0x0123456789abcdefull ^ (i << 20)}; return b; });
  std::vector<uint8_t> records(n * 45);                                                        // 37-byte messages, 45 bytes apart
  for (size_t i = 0; i < records.size(); ++i) records[i] = (uint8_t)(i * 131 + (i >> 8));
  const hip::messages m(records.data(), n, 37, 45);
  W256 px; hip::mask ok;
  const auto sig = CG::schnorr_sign(d, m, px, ok);
  EXPECT_TRUE(all(ok));
  EXPECT_TRUE(all(px == CG::scalar_mult_base_affine(d).x()));
  EXPECT_TRUE(all(CG::schnorr_verify(px, m, sig.first, sig.second)));
  records[36] ^= 1;                                                                            // the last byte of message 0
  const hip::messages changed(records.data(), n, 37, 45);
  const hip::mask v = CG::schnorr_verify(px, changed, sig.first, sig.second);
  EXPECT_TRUE(!v.get(0) && v.get(1) && v.get(n - 1));
  EXPECT_TRUE(none(CG::schnorr_verify(sig.first, m, sig.first, sig.second)));                  // another key
  // a key outside [1, n): the lane is refused, nothing is signed
  W256 pz; hip::mask okz;
  const auto bad = CG::schnorr_sign(W256(n, bignum_256{}), m, pz, okz);
  EXPECT_TRUE(none(okz) && bad.first.get(0) == bignum_256{} && bad.second.get(0) == bignum_256{} && pz.get(0) == bignum_256{});
  bool refused = false;                                                                        // operands of different length are refused before the device sees them
  try { (void)CG::schnorr_sign(W256(n - 1, bignum_256::from(5)), m, pz, okz); } catch (std::exception const&) { refused = true; }
  EXPECT_TRUE(refused);
}

int main() { return mini::run_all(); }
