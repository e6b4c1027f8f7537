// bip32_tests.cpp -- SHA-512, HMAC-SHA-512 and BIP-32 key derivation through the C++ host API (hip::sha512 / hmac_sha512,
// curve_group<curve_secp256k1>::bip32_master / bip32_ckd_priv / bip32_ckd_pub / bip32_derive_priv): BIP-32's test vector 1 level by level and as one path, and
// CKDpub of k G against CKDpriv of k.  Built and run by tests/test_cpp_bip32.py; the harness is mini_test.h.
#include <ecsimd/ecsimd.h>
#include "mini_test.h"

using namespace ecsimd;
using namespace ecsimd::literals;

namespace {
using W256 = wide_bignum<bignum_256>;
using CG = curve_group<curve_secp256k1>;
template <size_t N> bignum_256 bn(std::array<uint8_t, N> const& be) { return bn_from_bytes_BE<bignum_256>(be); }
// the members exist for secp256k1 only
template <class C> concept has_bip32 = requires(W256 const& a, W256& o, wide_curve_point<C> const& q, hip::messages const& s, hip::mask& m, std::vector<uint32_t> const& path) {
  curve_group<C>::bip32_master(s, o, m); curve_group<C>::bip32_ckd_priv(a, a, 1u, o, m); curve_group<C>::bip32_ckd_pub(q, a, 1u, o, m); curve_group<C>::bip32_derive_priv(a, a, path, o, m);
};
static_assert(has_bip32<curve_secp256k1> && !has_bip32<curve_nist_p256>);
constexpr uint32_t H = 0x80000000u;
}  // namespace

TEST(Bip32, Sha512KnownAnswer) {
  const hip::messages abc(std::vector<std::string>(default_lanes, std::string("abc")));
  const auto want = "ddaf35a193617abacc417349ae20413112e6fa4e89a97ea20a9eeee64b55d39a2192992a274fc1a836ba3c23a3feebbd454d4423643ce80e2a9ac94fa54ca49f"_hex;
  const auto got = hip::sha512(abc).host();
  EXPECT_TRUE(std::equal(want.begin(), want.end(), got.front().begin()) && got.front() == got.back());
  // HMAC("Bitcoin seed", seed) is the master node of vector 1: IL || IR
  std::vector<uint8_t> seed(16);
  for (size_t i = 0; i < 16; ++i) seed[i] = (uint8_t)i;
  const hip::messages key(std::vector<std::string>(1, std::string("Bitcoin seed")));
  const auto node = hip::hmac_sha512(key, hip::messages(seed.data(), 1, 16, 16)).get(0);
  const auto k = "e8f32e723decf4051aefac8e2c93c9c5b214313817cdb01a1494b917c8436b35"_hex, c = "873dff81c02f525623fd1fe5167eac3a55a049de3d314bb42ee227ffed37d508"_hex;
  EXPECT_TRUE(std::equal(k.begin(), k.end(), node.begin()) && std::equal(c.begin(), c.end(), node.begin() + 32));
}

TEST(Bip32, TestVector1) {
  const size_t n = 3;                                          // the same seed on every lane
  std::vector<uint8_t> seeds(16 * n);
  for (size_t i = 0; i < seeds.size(); ++i) seeds[i] = (uint8_t)(i % 16);
  W256 c; hip::mask ok;
  W256 k = CG::bip32_master(hip::messages(seeds.data(), n, 16, 16), c, ok);
  EXPECT_TRUE(all(ok));
  EXPECT_TRUE(k.get(n - 1) == bn("e8f32e723decf4051aefac8e2c93c9c5b214313817cdb01a1494b917c8436b35"_hex));
  EXPECT_TRUE(c.get(n - 1) == bn("873dff81c02f525623fd1fe5167eac3a55a049de3d314bb42ee227ffed37d508"_hex));
  const W256 k0 = k, c0 = c;
  const std::vector<uint32_t> path = {H, 1, H + 2, 2, 1000000000};
  const bignum_256 keys[5] = {bn("edb2e14f9ee77d26dd93b4ecede8d16ed408ce149b6cd80b0715a2d911a0afea"_hex), bn("3c6cb8d0f6a264c91ea8b5030fadaa8e538b020f0a387421a12de9319dc93368"_hex),
                              bn("cbce0d719ecf7431d88e6a89fa1483e02e35092af60c042b1df2ff59fa424dca"_hex), bn("0f479245fb19a38a1954c5c7c0ebab2f9bdfd96a17563ef28a6a4b1a2a764ef4"_hex),
                              bn("471b76e389e528d6de6d816857e012c5455051cad6660850e58372a6c3e6e7c8"_hex)};
  const bignum_256 codes[5] = {bn("47fdacbd0f1097043b78c63c20c34ef4ed9a111d980047ad16282c7ae6236141"_hex), bn("2a7857631386ba23dacac34180dd1983734e444fdbf774041578e9b6adb37c19"_hex),
                               bn("04466b9cc8e161e966409ca52986c584f07e9dc81f735db683c3ff6ec7b1503f"_hex), bn("cfb71883f01676f587d023cc53a35bc7f88f724b1f8c2892ac1275ac822a3edd"_hex),
                               bn("c783e67b921d2beb8f6b389cc646d7263b4145701dadd2161548a8b078e65e9e"_hex)};
  for (size_t level = 0; level < path.size(); ++level) {
    W256 cc;
    k = CG::bip32_ckd_priv(k, c, path[level], cc, ok);
    c = cc;
    EXPECT_TRUE(all(ok));
    EXPECT_TRUE(k.get(0) == keys[level] && k.get(n - 1) == keys[level]);
    EXPECT_TRUE(c.get(0) == codes[level] && c.get(n - 1) == codes[level]);
  }
  W256 cd;
  const W256 kd = CG::bip32_derive_priv(k0, c0, path, cd, ok);
  EXPECT_TRUE(all(ok) && kd.get(1) == keys[4] && cd.get(1) == codes[4]);
  // the parent fingerprint of m/0': the first four bytes of HASH160(serP(m G))
  const auto fp = CG::btc_pubkey_hash(CG::scalar_mult_base_affine(k0)).get(0);
  EXPECT_TRUE(fp[0] == 0x34 && fp[1] == 0x42 && fp[2] == 0x19 && fp[3] == 0x3e);
}

TEST(Bip32, CkdPubAgainstCkdPriv) {
  const size_t n = 300;
  const W256 k(n, [](size_t i, size_t) { bignum_256 b; b.limbs = {0x9e3779b97f4a7c15ull * (i + 1), i * 77, ~i, 0x0123456789abcdefull ^ (i << 20)}; return b; });
  const W256 c(n, [](size_t i, size_t) { bignum_256 b; b.limbs = {i, ~i * 3, i << 40, 0xfedcba9876543210ull + i}; return b; });
  std::vector<uint32_t> idx(n);
  for (size_t i = 0; i < n; ++i) idx[i] = (uint32_t)(i * 2654435761u) & 0x7fffffffu;
  const hip::indices index(idx);
  W256 cpriv, cpub; hip::mask ok, pok;
  const W256 child = CG::bip32_ckd_priv(k, c, index, cpriv, ok);
  EXPECT_TRUE(all(ok));
  const auto want = CG::scalar_mult_base_affine(child);
  const auto got = CG::bip32_ckd_pub(CG::scalar_mult_base_affine(k), c, index, cpub, pok);
  EXPECT_TRUE(all(pok));
  for (size_t i : {size_t(0), size_t(1), n / 2, n - 1}) {
    EXPECT_TRUE(got.x().get(i) == want.x().get(i) && got.y().get(i) == want.y().get(i) && cpub.get(i) == cpriv.get(i));
  }
  // a hardened index has no public derivation; with the promise of hardened indices a lane that is not is refused
  (void)CG::bip32_ckd_pub(CG::scalar_mult_base_affine(k), c, H, cpub, pok);
  EXPECT_TRUE(pok.count() == 0 && cpub.get(0) == bignum_256::from(0));
  const W256 none = CG::bip32_ckd_priv(k, c, index, cpriv, ok, ECSIMD_HIP_BIP32_ALL_HARDENED);
  EXPECT_TRUE(ok.count() == 0 && none.get(0) == bignum_256::from(0));
}

int main() { return mini::run_all(); }
