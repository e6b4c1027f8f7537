// ecdsa_recover_tests.cpp -- sign, recover, compare through the C++ host API (curve_group<Curve>::ecdsa_sign_recoverable / ecdsa_recover).
// Built and run by tests/test_cpp_ecdsa_recover.py on the GPU box; the harness is mini_test.h.
#include <ecsimd/ecsimd.h>
#include "mini_test.h"

using namespace ecsimd;
using namespace ecsimd::literals;

namespace {
using W256 = wide_bignum<bignum_256>;
template <size_t N> W256 splat(std::array<uint8_t, N> const& be) { return W256{bn_from_bytes_BE<bignum_256>(be)}; }
template <size_t N> W256 lanes(std::array<uint8_t, N> const& l0, std::array<uint8_t, N> const& l1, std::array<uint8_t, N> const& l2, std::array<uint8_t, N> const& l3) {
  const std::array<uint8_t, N> be[4] = {l0, l1, l2, l3};
  return W256{[&](size_t i, size_t) { return bn_from_bytes_BE<bignum_256>(be[i % 4]); }};
}
}  // namespace

TEST(EcdsaRecover, Rfc6979KeyComesBack) {
  // RFC 6979 A.2.5 (P-256, SHA-256): "sample" and "test" signed with the RFC's own nonces; the key that comes back is the RFC's public key
  using CG = curve_group<curve_nist_p256>; using WCP = wide_curve_point<curve_nist_p256>;
  const auto qx = "60FED4BA255A9D31C961EB74C6356D68C049B8923B61FA6CE669622E60F29FB6"_hex, qy = "7903FE1008B8BC99A41AE9E95628BC64F2F1B20C2D7E9F5177A3C294D4462299"_hex;
  const auto x = "C9AFA9D845BA75166B5C215767B1D6934E50C3DB36E89B127B8A622B120F6721"_hex;
  const auto e1 = "AF2BDBE1AA9B6EC1E2ADE1D694F41FC71A831D0268E9891562113D8A62ADD1BF"_hex, e2 = "9F86D081884C7D659A2FEAA0C55AD015A3BF4F1B2B0B822CD15D6C15B0F00A08"_hex;
  const auto k1 = "A6E3C57DD01ABE90086538398355DD4C3B17AA873382B0F24D6129493D8AAD60"_hex, k2 = "D16B6AE827F17175E040871A1C7EC3500192C4C92677336EC2537ACAEE0008E0"_hex;
  const auto r1 = "EFD48B2AACB6A8FD1140DD9CD45E81D69D2C877B56AAF991C34D0EA84EAF3716"_hex, s1 = "F7CB1C942D657C41D436C7A1B6E29F65F3E900DBB9AFF4064DC4AB2F843ACDA8"_hex;
  const auto zero = "0000000000000000000000000000000000000000000000000000000000000000"_hex;
  const auto e = lanes(e1, e2, e1, e2);
  hip::mask v, ok, rok;
  const auto sig = CG::ecdsa_sign_recoverable(e, splat(x), lanes(k1, k2, zero, k1), v, ok);
  const auto so = ok.host(), vh = v.host();
  EXPECT_TRUE(so[0] == 1 && so[1] == 1 && so[2] == 0 && so[3] == 1);
  EXPECT_TRUE(sig.first.get(0) == bn_from_bytes_BE<bignum_256>(r1) && sig.second.get(0) == bn_from_bytes_BE<bignum_256>(s1));
  EXPECT_TRUE(vh[0] <= 3 && vh[1] <= 3 && vh[2] == 0 && vh[3] <= 3);
  const WCP Q = CG::ecdsa_recover(e, sig.first, sig.second, v, rok);
  const auto ro = rok.host();
  EXPECT_TRUE(ro[0] == 1 && ro[1] == 1 && ro[2] == 0 && ro[3] == 1);
  for (size_t i : {0u, 1u, 3u}) EXPECT_TRUE(Q.x().get(i) == bn_from_bytes_BE<bignum_256>(qx) && Q.y().get(i) == bn_from_bytes_BE<bignum_256>(qy));
  EXPECT_TRUE(Q.x().get(2) == bignum_256{} && Q.y().get(2) == bignum_256{});                    // the refused lane: r = s = 0, no key
  // the same signatures in low-s form: still the same key, and the plain call's signature where s was low already
  hip::mask v2, ok2, rok2;
  const auto low = CG::ecdsa_sign_recoverable(e, splat(x), lanes(k1, k2, zero, k1), v2, ok2, true);
  const WCP Q2 = CG::ecdsa_recover(e, low.first, low.second, v2, rok2);
  EXPECT_TRUE(rok2.count() == 3 && Q2.x().get(0) == Q.x().get(0) && Q2.y().get(0) == Q.y().get(0) && Q2.x().get(1) == Q.x().get(1));
  EXPECT_TRUE(!(low.second.get(0) == sig.second.get(0)) && v2.host()[0] == (vh[0] ^ 1));        // s1 = F7CB... is above n / 2
  EXPECT_TRUE(low.second.get(1) == sig.second.get(1) && v2.host()[1] == vh[1]);                  // s2 = 019F... is not
  EXPECT_TRUE(CG::ecdsa_verify(e, low.first, low.second, WCP{splat(qx), splat(qy)}).count() == 3);
}

TEST(EcdsaRecover, Secp256k1RoundTripOverManyLanes) {
  using CG = curve_group<curve_secp256k1>;
  const size_t n = 300;
  const W256 d(n, [](size_t i, size_t) { bignum_256 b; b.limbs = {0x9e3779b97f4a7c15ull * (i + 1), i * 77, ~i, 0x0123456789abcdefull ^ (i << 20)}; return b; });
  const W256 k(n, [](size_t i, size_t) { bignum_256 b; b.limbs = {0xd1342543de82ef95ull * (i + 3), i * 131, ~(i << 7), 0x7edcba9876543210ull ^ (i << 33)}; return b; });
  const W256 e(n, [](size_t i, size_t) { bignum_256 b; b.limbs = {i, ~i * 3, 0xa5a5a5a5a5a5a5a5ull + i, 0xffffffffffffffffull - i}; return b; });
  const auto pub = CG::scalar_mult_base_affine(d);
  hip::mask v, ok, rok;
  const auto sig = CG::ecdsa_sign_recoverable(e, d, k, v, ok, true);
  EXPECT_TRUE(all(ok));
  const auto Q = CG::ecdsa_recover(e, sig.first, sig.second, v, rok);
  EXPECT_TRUE(all(rok) && all(Q == pub));
  EXPECT_TRUE(all(CG::ecdsa_verify(e, sig.first, sig.second, pub)));
  bool refused = false;                                                                          // operands of different length are refused before the device sees them
  try { (void)CG::ecdsa_recover(e, sig.first, sig.second, hip::mask(n - 1), rok); } catch (std::exception const&) { refused = true; }
  EXPECT_TRUE(refused);
}

int main() { return mini::run_all(); }
