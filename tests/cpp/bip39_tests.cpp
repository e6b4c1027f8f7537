// bip39_tests.cpp -- PBKDF2-HMAC-SHA-512 and the BIP-39 seed through the C++ host API (hip::pbkdf2_hmac_sha512, hip::bip39_seed,
// curve_group<curve_secp256k1>::bip39_master): the published BIP-39 vector with and without its passphrase on every lane, its BIP-32 master key, the first node
// below it against bip32_master on the same seed, and one PBKDF2 value with a salt per lane and with one salt for the call.  Built and run by
// tests/test_cpp_bip39.py; the harness is mini_test.h.
#include <ecsimd/ecsimd.h>
#include "mini_test.h"

using namespace ecsimd;
using namespace ecsimd::literals;

namespace {
using W256 = wide_bignum<bignum_256>;
using CG = curve_group<curve_secp256k1>;
template <size_t N> bignum_256 bn(std::array<uint8_t, N> const& be) { return bn_from_bytes_BE<bignum_256>(be); }
// the member exists for secp256k1 only
template <class C> concept has_bip39 = requires(hip::messages const& s, W256& o, hip::mask& m) { curve_group<C>::bip39_master(s, s, o, m); };
static_assert(has_bip39<curve_secp256k1> && !has_bip39<curve_nist_p256>);
const std::string SENTENCE = "abandon abandon abandon abandon abandon abandon abandon abandon abandon abandon abandon about";
template <size_t N> bool same(std::vector<uint8_t> const& got, std::array<uint8_t, N> const& want) { return got.size() == N && std::equal(want.begin(), want.end(), got.begin()); }
}  // namespace

TEST(Bip39, PublishedSeeds) {
  const size_t n = 67;                                         // a whole wave and a partial one
  const hip::messages words(std::vector<std::string>(n, SENTENCE));
  const auto with = hip::bip39_seed(words, hip::messages(std::vector<std::string>(1, std::string("TREZOR")))).host();
  const auto each = hip::bip39_seed(words, hip::messages(std::vector<std::string>(n, std::string("TREZOR")))).host();
  const auto without = hip::bip39_seed(words, hip::messages(nullptr, 1, 0, 0)).host();
  const auto s1 = "c55257c360c07c72029aebc1b53c05ed0362ada38ead3e3e9efa3708e53495531f09a6987599d18264c1e1c92f2cf141630c7a3c4ab7c81b2f001698e7463b04"_hex;
  const auto s0 = "5eb00bbddcf069084889a8ab9155568165f5c453ccb85e70811aaed6f6da5fc19a5ac40b389cd370d086206dec8aa6c43daea6690f20ad3d8d48b2d2ce9e38e4"_hex;
  EXPECT_TRUE(with.size() == n && same(with.front(), s1) && same(with.back(), s1) && each == with);
  EXPECT_TRUE(same(without.front(), s0) && same(without.back(), s0));
}

TEST(Bip39, MasterKey) {
  const size_t n = 3;
  const hip::messages words(std::vector<std::string>(n, SENTENCE)), phrase(std::vector<std::string>(1, std::string("TREZOR")));
  W256 c, c2; hip::mask ok, ok2;
  const W256 k = CG::bip39_master(words, phrase, c, ok);
  EXPECT_TRUE(all(ok));
  EXPECT_TRUE(k.get(0) == bn("cbedc75b0d6412c85c79bc13875112ef912fd1e756631b5a00330866f22ff184"_hex) && k.get(n - 1) == k.get(0));
  // the same through the seed's bytes on the host
  const auto seed = hip::bip39_seed(words, phrase).host();
  std::vector<uint8_t> flat;
  for (auto const& s : seed) flat.insert(flat.end(), s.begin(), s.end());
  const W256 k2 = CG::bip32_master(hip::messages(flat.data(), n, 64, 64), c2, ok2);
  EXPECT_TRUE(all(ok2) && k2.get(1) == k.get(1) && c2.get(1) == c.get(1));
}

TEST(Bip39, Pbkdf2KnownAnswer) {
  const size_t n = 5;
  const hip::messages pw(std::vector<std::string>(n, std::string("password")));
  const auto want = "867f70cf1ade02cff3752599a3a53dc4af34c7a669815ae5d513554e1c8cf252c02d470a285a0501bad999bfe943c08f050235d7d68b1da55e63f73b60a57fce"_hex;
  const auto one = hip::pbkdf2_hmac_sha512(pw, hip::messages(std::vector<std::string>(1, std::string("salt"))), 1, 64).host();
  const auto each = hip::pbkdf2_hmac_sha512(pw, hip::messages(std::vector<std::string>(n, std::string("salt"))), 1, 64).host();
  EXPECT_TRUE(same(one.front(), want) && same(one.back(), want) && one == each);
  // a shorter key is a prefix of a longer one's first block
  const auto head = hip::pbkdf2_hmac_sha512(pw, hip::messages(std::vector<std::string>(1, std::string("salt"))), 1, 20).host();
  EXPECT_TRUE(head.front().size() == 20 && std::equal(head.front().begin(), head.front().end(), want.begin()));
}

int main() { return mini::run_all(); }
