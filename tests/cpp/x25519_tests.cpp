// x25519_tests.cpp -- X25519 through the C++ host API (hip::x25519, hip::x25519_base, hip::x25519_from_ed25519_pk, hip::x25519_from_ed25519_seed): RFC 7748
// section 6.1 both ways on a whole wave and a partial one, the refusal of a small-order peer through `ok`, and the two conversions against each other.
// Built and run by tests/test_cpp_x25519.py; the harness is mini_test.h.
#include <ecsimd/ecsimd.h>
#include <ecsimd/x25519.h>
#include "mini_test.h"

using namespace ecsimd;
using namespace ecsimd::literals;

namespace {
template <size_t N> std::vector<uint8_t> vec(std::array<uint8_t, N> const& a) { return std::vector<uint8_t>(a.begin(), a.end()); }
const auto A = vec("77076d0a7318a57d3c16c17251b26645df4c2f87ebc0992ab177fba51db92c2a"_hex), A_PUB = vec("8520f0098930a754748b7ddcb43ef75a0dbf3a0d26381af4eba4a98eaa9b4e6a"_hex);
const auto B = vec("5dab087e624a8a4b79e17f8b83800ee66f3bb1292618b6fd1c2f8b27ff88e0eb"_hex), B_PUB = vec("de9edb7d7b7dc1b4d35b61c2ece435373f8343c85b78674dadfc7e146f882b4f"_hex);
const auto SHARED = vec("4a5d9d5ba4ce2de1728e3bf480350f25e07e21c947d19e3376f09b3c1e161742"_hex);
}  // namespace

TEST(X25519, Rfc7748DiffieHellmanBothWays) {
  const size_t n = 67;                                         // a whole wave and a partial one
  std::vector<std::vector<uint8_t>> mine, theirs, pubs;
  for (size_t i = 0; i < n; ++i) { mine.push_back(i % 2 ? B : A); theirs.push_back(i % 2 ? A : B); pubs.push_back(i % 2 ? B_PUB : A_PUB); }
  const hip::byte_records sk(mine, 32), peer_sk(theirs, 32);
  const auto pk = hip::x25519_base(sk), peer_pk = hip::x25519_base(peer_sk);
  EXPECT_TRUE(pk.host() == pubs);
  hip::mask ok;
  const auto s1 = hip::x25519(sk, peer_pk, &ok), s2 = hip::x25519(peer_sk, pk);
  EXPECT_TRUE(s1.host() == std::vector<std::vector<uint8_t>>(n, SHARED));
  EXPECT_TRUE(s2.host() == s1.host());
  EXPECT_TRUE(ok.host() == std::vector<uint8_t>(n, 1));
}

TEST(X25519, SmallOrderPeerIsRefusedThroughOk) {
  std::vector<std::vector<uint8_t>> us(4, std::vector<uint8_t>(32, 0));
  us[1][0] = 1;                                                // u = 1
  us[2] = B_PUB;
  us[3] = std::vector<uint8_t>(32, 0xff); us[3][0] = 0xec;     // p - 1 with bit 255 set
  hip::mask ok;
  const auto out = hip::x25519(hip::byte_records(std::vector<std::vector<uint8_t>>(4, A), 32), hip::byte_records(us, 32), &ok).host();
  const std::vector<uint8_t> zero(32, 0);
  EXPECT_TRUE(ok.host() == (std::vector<uint8_t>{0, 0, 1, 0}));
  EXPECT_TRUE(out[0] == zero && out[1] == zero && out[2] == SHARED && out[3] == zero);
}

TEST(X25519, Ed25519KeysConvertConsistently) {
  const auto seed = vec("9d61b19deffd5a60ba844af492ec2cc44449c5697b326919703bac031cae7f60"_hex);      // RFC 8032 7.1 TEST 1
  std::vector<std::vector<uint8_t>> seeds(5, seed);
  for (size_t i = 1; i < 5; ++i) seeds[i][0] ^= (uint8_t)i;
  const hip::byte_records sd(seeds, 32);
  const auto [u, ok] = hip::x25519_from_ed25519_pk(hip::ed25519_pubkey(sd));
  EXPECT_TRUE(ok.host() == std::vector<uint8_t>(5, 1));
  EXPECT_TRUE(u.host() == hip::x25519_base(hip::x25519_from_ed25519_seed(sd)).host());
  std::vector<std::vector<uint8_t>> ident(1, std::vector<uint8_t>(32, 0)); ident[0][0] = 1;             // the identity: small order
  const auto [u0, ok0] = hip::x25519_from_ed25519_pk(hip::byte_records(ident, 32));
  EXPECT_TRUE(ok0.host() == std::vector<uint8_t>{0} && u0.get(0) == std::vector<uint8_t>(32, 0));
}

int main() { return mini::run_all(); }
