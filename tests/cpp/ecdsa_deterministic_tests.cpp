// ecdsa_deterministic_tests.cpp -- hash, sign deterministically, check through the C++ host API (hip::sha256, curve_group<Curve>::ecdsa_sign_deterministic)
// on one built-in and one registered curve.  Built and run by tests/test_cpp_ecdsa_deterministic.py on the GPU box; the harness is mini_test.h.
#include <ecsimd/ecsimd.h>
#include "mini_test.h"

using namespace ecsimd;
using namespace ecsimd::literals;

namespace {
using W256 = wide_bignum<bignum_256>;
template <size_t N> bignum_256 bn(std::array<uint8_t, N> const& be) { return bn_from_bytes_BE<bignum_256>(be); }

// brainpoolP256r1 (RFC 5639 3.4) with its order: registered with the engine on first use
struct curve_brainpoolp256r1_n {
  using bn_type = bignum_256;
  using P  = bn256_constant<0xa9fb57dba1eea9bcull, 0x3e660a909d838d72ull, 0x6e3bf623d5262028ull, 0x2013481d1f6e5377ull>;
  using A  = bn256_constant<0x7d5a0975fc2c3057ull, 0xeef67530417affe7ull, 0xfb8055c126dc5c6cull, 0xe94a4b44f330b5d9ull>;
  using B  = bn256_constant<0x26dc5c6ce94a4b44ull, 0xf330b5d9bbd77cbfull, 0x958416295cf7e1ceull, 0x6bccdc18ff8c07b6ull>;
  using Gx = bn256_constant<0x8bd2aeb9cb7e57cbull, 0x2c4b482ffc81b7afull, 0xb9de27e1e3bd23c2ull, 0x3a4453bd9ace3262ull>;
  using Gy = bn256_constant<0x547ef835c3dac4fdull, 0x97f8461a14611dc9ull, 0xc27745132ded8e54ull, 0x5c1d54c72f046997ull>;
  using N  = bn256_constant<0xa9fb57dba1eea9bcull, 0x3e660a909d838d71ull, 0x8c397aa3b561a6f7ull, 0x901e0e82974856a7ull>;
};
}  // namespace

TEST(EcdsaDeterministic, Rfc6979KnownAnswersFromTheMessages) {
  // RFC 6979 A.2.5 (P-256, SHA-256): "sample" and "test" hashed and signed on the device; r and s are the RFC's
  using CG = curve_group<curve_nist_p256>; using WCP = wide_curve_point<curve_nist_p256>;
  const auto x = "C9AFA9D845BA75166B5C215767B1D6934E50C3DB36E89B127B8A622B120F6721"_hex;
  const auto qx = "60FED4BA255A9D31C961EB74C6356D68C049B8923B61FA6CE669622E60F29FB6"_hex, qy = "7903FE1008B8BC99A41AE9E95628BC64F2F1B20C2D7E9F5177A3C294D4462299"_hex;
  // (a wide built from one value has default_lanes lanes: each message is hashed that many times)
  const W256 e1 = hip::sha256(hip::messages(std::vector<std::string>(default_lanes, "sample"))), e2 = hip::sha256(hip::messages(std::vector<std::string>(default_lanes, "test")));
  EXPECT_TRUE(e1.get(0) == bn("AF2BDBE1AA9B6EC1E2ADE1D694F41FC71A831D0268E9891562113D8A62ADD1BF"_hex));
  EXPECT_TRUE(e2.get(0) == bn("9F86D081884C7D659A2FEAA0C55AD015A3BF4F1B2B0B822CD15D6C15B0F00A08"_hex));
  hip::mask v, ok, kok;
  const auto s1 = CG::ecdsa_sign_deterministic(e1, W256{bn(x)}, v, ok);
  EXPECT_TRUE(all(ok) && s1.first.get(0) == bn("EFD48B2AACB6A8FD1140DD9CD45E81D69D2C877B56AAF991C34D0EA84EAF3716"_hex) &&
              s1.second.get(0) == bn("F7CB1C942D657C41D436C7A1B6E29F65F3E900DBB9AFF4064DC4AB2F843ACDA8"_hex));
  const auto s2 = CG::ecdsa_sign_deterministic(e2, W256{bn(x)}, v, ok);
  EXPECT_TRUE(all(ok) && s2.first.get(0) == bn("F1ABB023518351CD71D881567B1EA663ED3EFCF6C5132B354F28D3B0B7D38367"_hex) &&
              s2.second.get(0) == bn("019F4113742A2B14BD25926B49C649155F267E60D3814B4C0CC84250E46F0083"_hex));
  EXPECT_TRUE(CG::rfc6979_nonce(e1, W256{bn(x)}, kok).get(0) == bn("A6E3C57DD01ABE90086538398355DD4C3B17AA873382B0F24D6129493D8AAD60"_hex) && all(kok));
  EXPECT_TRUE(all(CG::ecdsa_verify(e2, s2.first, s2.second, WCP{W256{bn(qx)}, W256{bn(qy)}})));
  // a record array: 4-byte messages 8 bytes apart give the digests of the packed ones
  const std::string records = std::string("test") + "\x01\x02\x03\x04" + "abcd" + "\xff\xff\xff\xff";
  const W256 strided = hip::sha256(hip::messages(reinterpret_cast<const uint8_t*>(records.data()), 2, 4, 8));
  const W256 packed = hip::sha256(hip::messages(std::vector<std::string>{"test", "abcd"}));
  EXPECT_TRUE(all(strided == packed) && strided.get(0) == e2.get(0) && !(strided.get(1) == e2.get(0)));
  // a key outside [1, n): the lane is refused, nothing is signed
  const auto bad = CG::ecdsa_sign_deterministic(e1, W256{bignum_256{}}, v, ok);
  EXPECT_TRUE(none(ok) && bad.first.get(0) == bignum_256{} && bad.second.get(0) == bignum_256{});
}

TEST(EcdsaDeterministic, RegisteredCurveSignsLikeTheChainAndVerifies) {
  using CG = curve_group<curve_brainpoolp256r1_n>;
  EXPECT_TRUE(CG::curve_id() >= ECSIMD_HIP_FIRST_REGISTERED_CURVE);
  const size_t n = 300;                                                                          // a third of the lanes draw more than one candidate on this curve
  const W256 d(n, [](size_t i, size_t) { bignum_256 b; b.limbs = {0x9e3779b97f4a7c15ull * (i + 1), i * 77, ~i, 0x0123456789abcdefull ^ (i << 20)}; return b; });
  std::vector<std::string> msgs;
  for (size_t i = 0; i < n; ++i) msgs.push_back("message number " + std::to_string(1000 + i));
  const W256 e = hip::sha256(hip::messages(msgs));
  const auto pub = CG::scalar_mult_base_affine(d);
  for (bool low_s : {false, true}) {
    hip::mask v, ok, kok, v2, ok2, rok;
    const auto sig = CG::ecdsa_sign_deterministic(e, d, v, ok, low_s);
    EXPECT_TRUE(all(ok));
    const W256 k = CG::rfc6979_nonce(e, d, kok);
    const auto chain = CG::ecdsa_sign_recoverable(e, d, k, v2, ok2, low_s);
    EXPECT_TRUE(all(kok) && all(ok2) && all(sig.first == chain.first) && all(sig.second == chain.second) && all(v == v2));
    EXPECT_TRUE(all(CG::ecdsa_verify(e, sig.first, sig.second, pub)));
    const auto Q = CG::ecdsa_recover(e, sig.first, sig.second, v, rok);
    EXPECT_TRUE(all(rok) && all(Q == pub));
  }
  bool refused = false;                                                                          // operands of different length are refused before the device sees them
  hip::mask v, ok;
  try { (void)CG::ecdsa_sign_deterministic(e, W256(n - 1, bignum_256::from(5)), v, ok); } catch (std::exception const&) { refused = true; }
  EXPECT_TRUE(refused);
}

int main() { return mini::run_all(); }
