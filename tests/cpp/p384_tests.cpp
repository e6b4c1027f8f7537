// p384_tests.cpp -- NIST P-384 through the C++ host API (hip::p384_sha384, p384_pubkey, p384_ecdh, p384_ecdsa_sign, p384_ecdsa_verify): RFC 6979 A.2.6 with
// SHA-384 -- the records tests/golden/p384_vectors.json opens with -- on a whole wave and a partial one, a refused key through `ok`, and ECDH both ways.
// Built and run by tests/test_cpp_p384.py; the harness is mini_test.h.
#include <ecsimd/ecsimd.h>
#include <ecsimd/p384.h>
#include "mini_test.h"

using namespace ecsimd;
using namespace ecsimd::literals;

namespace {
template <size_t N> std::vector<uint8_t> vec(std::array<uint8_t, N> const& a) { return std::vector<uint8_t>(a.begin(), a.end()); }
std::vector<uint8_t> cat(std::vector<uint8_t> a, std::vector<uint8_t> const& b) { a.insert(a.end(), b.begin(), b.end()); return a; }
const auto X = vec("6B9D3DAD2E1B8C1C05B19875B6659F4DE23C3B667BF297BA9AA47740787137D896D5724E4C70A825F872C9EA60D2EDF5"_hex);
const auto UX = vec("EC3A4E415B4E19A4568618029F427FA5DA9A8BC4AE92E02E06AAE5286B300C64DEF8F0EA9055866064A254515480BC13"_hex);
const auto UY = vec("8015D9B72D7D57244EA8EF9AC0C621896708A59367F9DFB9F54CA84B3F1C9DB1288B231C3AE0D4FE7344FD2533264720"_hex);
const auto R_SAMPLE = vec("94EDBB92A5ECB8AAD4736E56C691916B3F88140666CE9FA73D64C4EA95AD133C81A648152E44ACF96E36DD1E80FABE46"_hex);
const auto S_SAMPLE = vec("99EF4AEB15F178CEA1FE40DB2603138F130E740A19624526203B6351D0A3A94FA329C145786E679E7B82C71A38628AC8"_hex);
const auto R_TEST = vec("8203B63D3C853E8D77227FB377BCF7B7B772E97892A80F36AB775D509D7A5FEB0542A7F0812998DA8F1DD3CA3CF023DB"_hex);
const auto S_TEST = vec("DDD0760448D42D8A43AF45AF836FCE4DE8BE06B485E9B61B827C2F13173923E06A739F040649A667BF3B828246BAA5A5"_hex);
const auto SHA_SAMPLE = vec("9A9083505BC92276AEC4BE312696EF7BF3BF603F4BBD381196A029F340585312313BCA4A9B5B890EFEE42C77B1EE25FE"_hex);
}  // namespace

TEST(P384, Rfc6979SignaturesAndTheirVerdicts) {
  const size_t n = 67;                                         // a whole wave and a partial one
  std::vector<std::string> msgs;
  std::vector<std::vector<uint8_t>> keys(n, X), want_sig, want_pub(n, cat(UX, UY));
  for (size_t i = 0; i < n; ++i) { msgs.push_back(i % 2 ? "test\0\0" : "sample"); want_sig.push_back(i % 2 ? cat(R_TEST, S_TEST) : cat(R_SAMPLE, S_SAMPLE)); }
  std::vector<uint32_t> lens;
  for (size_t i = 0; i < n; ++i) lens.push_back(i % 2 ? 4 : 6);
  for (auto& m : msgs) m.resize(6, '\0');
  const hip::lengths ln(lens);
  const auto digest = hip::p384_sha384(hip::messages(msgs), &ln);
  EXPECT_TRUE(digest.get(0) == SHA_SAMPLE);
  const hip::byte_records d(keys, 48);
  const auto [pub, pub_ok] = hip::p384_pubkey(d);
  EXPECT_TRUE(pub.host() == want_pub);
  EXPECT_TRUE(pub_ok.host() == std::vector<uint8_t>(n, 1));
  const auto [sig, sig_ok] = hip::p384_ecdsa_sign(d, digest);
  EXPECT_TRUE(sig.host() == want_sig);
  EXPECT_TRUE(sig_ok.host() == std::vector<uint8_t>(n, 1));
  EXPECT_TRUE(hip::p384_ecdsa_verify(pub, digest, sig).host() == std::vector<uint8_t>(n, 1));
  auto bent = want_sig;
  for (size_t i = 0; i < n; i += 3) bent[i][95] ^= 1;
  std::vector<uint8_t> verdicts;
  for (size_t i = 0; i < n; ++i) verdicts.push_back(i % 3 ? 1 : 0);
  EXPECT_TRUE(hip::p384_ecdsa_verify(pub, digest, hip::byte_records(bent, 96)).host() == verdicts);
}

TEST(P384, RefusedKeysComeBackThroughOk) {
  std::vector<std::vector<uint8_t>> keys(3, std::vector<uint8_t>(48, 0));
  keys[1] = X;
  keys[2] = std::vector<uint8_t>(48, 0xff);                    // >= n
  const auto [pub, ok] = hip::p384_pubkey(hip::byte_records(keys, 48));
  EXPECT_TRUE(ok.host() == (std::vector<uint8_t>{0, 1, 0}));
  EXPECT_TRUE(pub.get(0) == std::vector<uint8_t>(96, 0) && pub.get(1) == cat(UX, UY) && pub.get(2) == std::vector<uint8_t>(96, 0));
}

TEST(P384, EcdhAgreesBothWays) {
  const size_t n = 5;
  std::vector<std::vector<uint8_t>> a(n, X), b(n, X);
  for (size_t i = 0; i < n; ++i) { a[i][47] ^= (uint8_t)(i + 1); b[i][0] ^= (uint8_t)(i + 1); }
  const hip::byte_records da(a, 48), db(b, 48);
  const auto pa = hip::p384_pubkey(da).first, pb = hip::p384_pubkey(db).first;
  const auto [z1, ok1] = hip::p384_ecdh(da, pb);
  const auto [z2, ok2] = hip::p384_ecdh(db, pa);
  EXPECT_TRUE(z1.host() == z2.host());
  EXPECT_TRUE(ok1.host() == std::vector<uint8_t>(n, 1) && ok2.host() == ok1.host());
  EXPECT_TRUE(z1.get(0) != std::vector<uint8_t>(48, 0));
  auto off = pb.host();
  off[2][95] ^= 1;                                             // off the curve
  const auto [z3, ok3] = hip::p384_ecdh(da, hip::byte_records(off, 96));
  EXPECT_TRUE(ok3.host() == (std::vector<uint8_t>{1, 1, 0, 1, 1}) && z3.get(2) == std::vector<uint8_t>(48, 0) && z3.get(1) == z1.get(1));
}

int main() { return mini::run_all(); }
