// ed25519_tests.cpp -- Ed25519 through the C++ host API (hip::ed25519_pubkey, hip::ed25519_sign, hip::ed25519_verify): RFC 8032 7.1 TEST 1-3 in one ragged
// batch on a whole wave and a partial one, and the rejects of the rule set (a changed message, a changed signature, s + L, a small-order key with the flag).
// Built and run by tests/test_cpp_ed25519.py; the harness is mini_test.h.
#include <ecsimd/ecsimd.h>
#include <ecsimd/ed25519.h>
#include "mini_test.h"

using namespace ecsimd;
using namespace ecsimd::literals;

namespace {
template <size_t N> std::vector<uint8_t> vec(std::array<uint8_t, N> const& a) { return std::vector<uint8_t>(a.begin(), a.end()); }
struct kat { std::vector<uint8_t> seed, pk, sig; std::string msg; };
std::vector<kat> rfc8032() {
  return {
      {vec("9d61b19deffd5a60ba844af492ec2cc44449c5697b326919703bac031cae7f60"_hex), vec("d75a980182b10ab7d54bfed3c964073a0ee172f3daa62325af021a68f707511a"_hex),
       vec("e5564300c360ac729086e2cc806e828a84877f1eb8e5d974d873e065224901555fb8821590a33bacc61e39701cf9b46bd25bf5f0595bbe24655141438e7a100b"_hex), std::string()},
      {vec("4ccd089b28ff96da9db6c346ec114e0f5b8a319f35aba624da8cf6ed4fb8a6fb"_hex), vec("3d4017c3e843895a92b70aa74d1b7ebc9c982ccf2ec4968cc0cd55f12af4660c"_hex),
       vec("92a009a9f0d4cab8720e820b5f642540a2b27b5416503f8fb3762223ebdb69da085ac1e43e15996e458f3613d0f11d8c387b2eaeb4302aeeb00d291612bb0c00"_hex), std::string("\x72")},
      {vec("c5aa8df43f9f837bedb7442f31dcb7b166d38535076f094b85ce3a2e0b4458f7"_hex), vec("fc51cd8e6218a1a38da47ed00230f0580816ed13ba3303ac5deb911548908025"_hex),
       vec("6291d657deec24024827e69c3abe01a30ce548a284743a445e3680d7db5ac3ac18ff9b538d16f290ae67f760984dc6594a7c15e9716ed28dc027beceea1ec40a"_hex), std::string("\xaf\x82")}};
}
}  // namespace

TEST(Ed25519, Rfc8032SignAndVerify) {
  const auto k = rfc8032();
  const size_t n = 67;                                         // a whole wave and a partial one
  std::vector<std::vector<uint8_t>> seeds, pks, sigs; std::vector<std::string> msgs;
  for (size_t i = 0; i < n; ++i) { seeds.push_back(k[i % 3].seed); pks.push_back(k[i % 3].pk); sigs.push_back(k[i % 3].sig); msgs.push_back(k[i % 3].msg); }
  const auto [m, lens] = hip::ragged(msgs);
  const hip::byte_records sd(seeds, 32);
  EXPECT_TRUE(hip::ed25519_pubkey(sd).host() == pks);
  const auto [sig, pk] = hip::ed25519_sign(sd, m, &lens);
  EXPECT_TRUE(sig.host() == sigs && pk.host() == pks);
  EXPECT_TRUE(hip::ed25519_verify(pk, m, sig, &lens).count() == n);
  EXPECT_TRUE(hip::ed25519_verify(pk, m, sig, &lens, true).count() == n);
}

TEST(Ed25519, Rejects) {
  const auto k = rfc8032();
  std::vector<std::vector<uint8_t>> pks(5, k[2].pk), sigs(5, k[2].sig);
  std::vector<std::string> msgs(5, k[2].msg);
  msgs[1][0] ^= 1;                                             // a changed message
  sigs[2][3] ^= 0x10;                                          // a changed R
  {                                                            // s + L: the same residue, refused
    const auto L = "edd3f55c1a631258d69cf7a2def9de1400000000000000000000000000000010"_hex;
    unsigned carry = 0;
    for (size_t j = 0; j < 32; ++j) { const unsigned v = sigs[3][32 + j] + L[j] + carry; sigs[3][32 + j] = (uint8_t)v; carry = v >> 8; }
    EXPECT_TRUE(carry == 0);
  }
  pks[4] = std::vector<uint8_t>(32, 0); pks[4][0] = 1;         // A = the identity, R = the identity, s = 0: accepted by default, refused with the flag
  sigs[4] = std::vector<uint8_t>(64, 0); sigs[4][0] = 1;
  const hip::messages m(msgs);
  const hip::byte_records pk(pks, 32), sig(sigs, 64);
  EXPECT_TRUE(hip::ed25519_verify(pk, m, sig).host() == (std::vector<uint8_t>{1, 0, 0, 0, 1}));
  EXPECT_TRUE(hip::ed25519_verify(pk, m, sig, nullptr, true).host() == (std::vector<uint8_t>{1, 0, 0, 0, 0}));
}

int main() { return mini::run_all(); }
