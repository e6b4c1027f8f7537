// keccak_tests.cpp -- Keccak-256 and the Ethereum members through the C++ host API (hip::keccak256, curve_group<curve_secp256k1>::eth_address / eth_recover):
// the known answers, a sign-and-recover round trip over a record array, and refusals.  Built and run by tests/test_cpp_keccak.py; the harness is mini_test.h.
#include <ecsimd/ecsimd.h>
#include "mini_test.h"

using namespace ecsimd;
using namespace ecsimd::literals;

namespace {
using W256 = wide_bignum<bignum_256>;
using CG = curve_group<curve_secp256k1>;
template <size_t N> bignum_256 bn(std::array<uint8_t, N> const& be) { return bn_from_bytes_BE<bignum_256>(be); }
// the two members exist for secp256k1 only
template <class C> concept has_eth = requires(W256 const& a, wide_curve_point<C> const& q, hip::mask const& v, hip::mask& ok) {
  curve_group<C>::eth_address(q); curve_group<C>::eth_recover(a, a, a, v, ok);
};
static_assert(has_eth<curve_secp256k1> && !has_eth<curve_nist_p256>);
hip::mask bytes_mask(std::vector<uint8_t> const& h) {
  hip::mask m(h.size());
  hip::check(ecsimd_hip_memcpy_h2d(hip::context(), m.data(), h.data(), h.size()), "h2d");
  return m;
}
}  // namespace

TEST(Keccak, KnownAnswers) {
  const W256 empty = hip::keccak256(hip::messages(std::vector<std::string>(default_lanes, std::string())));
  EXPECT_TRUE(empty.get(0) == bn("c5d2460186f7233c927e7db2dcc703c0e500b653ca82273b7bfad8045d85a470"_hex));
  const W256 abc = hip::keccak256(hip::messages(std::vector<std::string>(default_lanes, std::string("abc"))));
  EXPECT_TRUE(abc.get(0) == bn("4e03657aea45a94fc7d47ba826c8d667c0d1e6e33a64a036ec44f58fa12d6c45"_hex));
  EXPECT_TRUE(abc.get(default_lanes - 1) == abc.get(0));
  // the address of secret key 1
  const auto a = CG::eth_address(CG::scalar_mult_base_affine(W256{bignum_256::from(1)})).get(0);
  const auto want = "7e5f4552091a69125d5dfcb7b8c2659029395bdf"_hex;
  EXPECT_TRUE(std::equal(a.begin(), a.end(), want.begin()));
}

TEST(Keccak, SignAndRecoverOverARecordArray) {
  const size_t n = 300;
  const W256 d(n, [](size_t i, size_t) { bignum_256 b; b.limbs = {0x9e3779b97f4a7c15ull * (i + 1), i * 77, ~i, 0x0123456789abcdefull ^ (i << 20)}; return b; });
  std::vector<uint8_t> records(n * 160);                                                       // 150-byte messages (two blocks), 160 bytes apart
  for (size_t i = 0; i < records.size(); ++i) records[i] = (uint8_t)(i * 131 + (i >> 8));
  const W256 e = hip::keccak256(hip::messages(records.data(), n, 150, 160));
  hip::mask v, ok;
  const auto sig = CG::ecdsa_sign_deterministic(e, d, v, ok, true);
  EXPECT_TRUE(all(ok));
  const auto want = CG::eth_address(CG::scalar_mult_base_affine(d)).host();
  hip::mask rok;
  EXPECT_TRUE(CG::eth_recover(e, sig.first, sig.second, v, rok, ECSIMD_HIP_ETH_REQUIRE_LOW_S).host() == want);
  EXPECT_TRUE(all(rok));
  std::vector<uint8_t> vh = v.host();
  for (auto& b : vh) b += 27;
  vh[7] = 31;                                                                                  // not a value Ethereum knows
  const auto got = CG::eth_recover(e, sig.first, sig.second, bytes_mask(vh), rok).host();
  EXPECT_TRUE(!rok.get(7) && rok.count() == n - 1);
  EXPECT_TRUE(got[7] == hip::addresses::address{} && got[6] == want[6] && got[8] == want[8]);
  bool refused = false;                                                                        // operands of different length are refused before the device sees them
  try { (void)CG::eth_recover(e, W256(n - 1, bignum_256::from(5)), sig.second, v, rok); } catch (std::exception const&) { refused = true; }
  EXPECT_TRUE(refused);
}

int main() { return mini::run_all(); }
