// sm2_tests.cpp -- the SM2 signature scheme through the C++ host API (hip::sm3, sm2_za, sm2_digest, sm2_pubkey, sm2_sign_digest, sm2_verify, sm2_verify_digest
// on curve_sm2): the signature example of GB/T 32918.2 on the recommended curve -- the record tests/golden/sm2_vectors.json holds as "example" -- on a whole
// wave and a partial one, changed signatures and refused keys through their masks.  Built and run by tests/test_cpp_sm2.py; the harness is mini_test.h.
#include <ecsimd/ecsimd.h>
#include <ecsimd/curve_sm2.h>
#include <ecsimd/sm2.h>
#include "mini_test.h"

using namespace ecsimd;

namespace {
bignum_256 bn(const char* hex) {                                // 64 hexadecimal digits, most significant first
  bignum_256 r{};
  for (int i = 0; i < 64; ++i) {
    const char c = hex[i];
    const uint64_t v = c <= '9' ? c - '0' : (c | 0x20) - 'a' + 10;
    r.limbs[(63 - i) / 16] |= v << (4 * ((63 - i) % 16));
  }
  return r;
}
const bignum_256 D = bn("3945208F7B2144B13F36E38AC6D39F95889393692860B51A42FB81EF4DF7C5B8");
const bignum_256 K = bn("59276E27D506861A16680F3AD9C02DCCEF3CC1FA3CDBE4CE6D54B80DEAC1BC21");
const bignum_256 QX = bn("09F9DF311E5421A150DD7D161E4BC5C672179FAD1833FC076BB08FF356F35020");
const bignum_256 QY = bn("CCEA490CE26775A52DC6EA718CC1AA600AED05FBF35E084A6632F6072DA9AD13");
const bignum_256 E = bn("F0B43E94BA45ACCAACE692ED534382EB17E6AB5A19CE7B31F4486FDFC0D28640");
const bignum_256 R = bn("F5A03B0648D2C4630EEAC513E1BB81A15944DA3827D5B74143AC7EACEEE720B3");
const bignum_256 S = bn("B1B6AA29DF212FD8763182BC0D421CA1BB9038FD1F7F42D4840B69C485BBC1AA");
const bignum_256 SM3_ABC = bn("66c7f0f462eeedd9d1f2d46bdc10e4e24167c4875cf2f7a2297da02b8f4ba8e0");
using BN = hip::sm2_bn;
}  // namespace

TEST(Sm2, TheCurveTypeIsTheRegisteredCurve) {
  int id = -1;
  EXPECT_TRUE(ecsimd_sm2_curve(&id) == ECSIMD_HIP_OK);
  EXPECT_TRUE(id == hip_curve_id_of<curve_sm2>() && id >= 2);
}

TEST(Sm2, Sm3OfAbc) {
  const auto [m, lens] = hip::ragged({"abc", "abcX", "abcdefgh"});
  std::vector<uint32_t> three(3, 3);
  const hip::lengths ln(three);
  const auto e = hip::sm3(m, &ln).host();
  EXPECT_TRUE(e[0] == SM3_ABC && e[1] == SM3_ABC && e[2] == SM3_ABC);
  EXPECT_TRUE(hip::sm3(hip::messages(std::vector<std::string>{"abc", "abc"})).get(1) == SM3_ABC);
}

TEST(Sm2, TheStandardsExample) {
  const size_t n = 67;                                         // a whole wave and a partial one
  hip::mask key_ok, sig_ok;
  const auto Q = hip::sm2_pubkey<curve_sm2>(BN(n, D), key_ok);
  EXPECT_TRUE(Q.x().host() == std::vector<bignum_256>(n, QX) && Q.y().host() == std::vector<bignum_256>(n, QY));
  EXPECT_TRUE(key_ok.host() == std::vector<uint8_t>(n, 1));
  const hip::messages msgs(std::vector<std::string>(n, "message digest"));
  const auto e = hip::sm2_digest(Q, msgs);                     // the default identity
  EXPECT_TRUE(e.host() == std::vector<bignum_256>(n, E));
  EXPECT_TRUE(hip::sm2_digest(Q, msgs, hip::sm2_identity(std::string("1234567812345678"))).get(66) == E);
  EXPECT_TRUE(hip::sm2_digest(Q, msgs, hip::sm2_identity(hip::messages(std::vector<std::string>(n, "1234567812345678")))).get(65) == E);
  EXPECT_TRUE(!(hip::sm2_digest(Q, msgs, hip::sm2_identity(std::string("1234567812345679"))).get(0) == E));
  const BN k(n, K);
  const auto [r, s] = hip::sm2_sign_digest<curve_sm2>(e, BN(n, D), &k, sig_ok);
  EXPECT_TRUE(r.host() == std::vector<bignum_256>(n, R) && s.host() == std::vector<bignum_256>(n, S));
  EXPECT_TRUE(sig_ok.host() == std::vector<uint8_t>(n, 1));
  EXPECT_TRUE(hip::sm2_verify(Q, msgs, r, s).host() == std::vector<uint8_t>(n, 1));
  EXPECT_TRUE(hip::sm2_verify_digest(e, r, s, Q).host() == std::vector<uint8_t>(n, 1));
  auto bent = s.host();
  std::vector<uint8_t> verdicts;
  for (size_t i = 0; i < n; ++i) { if (i % 3 == 0) bent[i].limbs[0] ^= 1; verdicts.push_back(i % 3 ? 1 : 0); }
  EXPECT_TRUE(hip::sm2_verify(Q, msgs, r, BN(bent)).host() == verdicts);
  EXPECT_TRUE(hip::sm2_verify_digest(e, r, BN(bent), Q).host() == verdicts);
  // the deterministic nonce: another signature of the same digest, accepted all the same; the same one every time
  hip::mask det_ok;
  const auto [r2, s2] = hip::sm2_sign_digest<curve_sm2>(e, BN(n, D), nullptr, det_ok);
  const auto [r3, s3] = hip::sm2_sign_digest<curve_sm2>(e, BN(n, D), nullptr, det_ok);
  EXPECT_TRUE(det_ok.host() == std::vector<uint8_t>(n, 1) && !(r2.get(0) == R) && r2.host() == r3.host() && s2.host() == s3.host());
  EXPECT_TRUE(hip::sm2_verify(Q, msgs, r2, s2).host() == std::vector<uint8_t>(n, 1));
}

TEST(Sm2, RefusedKeysComeBackThroughOk) {
  const bignum_256 n = curve_sm2::N::value;
  bignum_256 nm1 = n, nm2 = n;
  nm1.limbs[0] -= 1; nm2.limbs[0] -= 2;
  hip::mask ok;
  const auto Q = hip::sm2_pubkey<curve_sm2>(BN(std::vector<bignum_256>{bignum_256{}, D, nm2, nm1, n}), ok);
  EXPECT_TRUE(ok.host() == (std::vector<uint8_t>{0, 1, 1, 0, 0}));
  EXPECT_TRUE(Q.x().get(0) == bignum_256{} && Q.x().get(1) == QX && Q.x().get(3) == bignum_256{} && Q.y().get(4) == bignum_256{});
  const BN e(5, E), k(5, K);
  const auto [r, s] = hip::sm2_sign_digest<curve_sm2>(e, BN(std::vector<bignum_256>{bignum_256{}, D, nm2, nm1, n}), &k, ok);
  EXPECT_TRUE(ok.host() == (std::vector<uint8_t>{0, 1, 1, 0, 0}));
  EXPECT_TRUE(r.get(1) == R && s.get(1) == S && r.get(3) == bignum_256{} && s.get(0) == bignum_256{});
}

int main() { return mini::run_all(); }
