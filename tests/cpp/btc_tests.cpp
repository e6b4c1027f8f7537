// btc_tests.cpp -- Bitcoin's hashes and the Taproot key tweaks through the C++ host API (hip::ripemd160 / hash160 / sha256d,
// curve_group<curve_secp256k1>::btc_pubkey_hash / xonly_tweak_add / taproot_tweak_pubkey / taproot_tweak_seckey): one published vector each, and a key-path
// spend signed by the tweaked key and verified under the output key.  Built and run by tests/test_cpp_btc.py; the harness is mini_test.h.
#include <ecsimd/ecsimd.h>
#include "mini_test.h"

using namespace ecsimd;
using namespace ecsimd::literals;

namespace {
using W256 = wide_bignum<bignum_256>;
using CG = curve_group<curve_secp256k1>;
template <size_t N> bignum_256 bn(std::array<uint8_t, N> const& be) { return bn_from_bytes_BE<bignum_256>(be); }
template <size_t N> bool same(hip::digests20::address const& a, std::array<uint8_t, N> const& want) { return N == 20 && std::equal(a.begin(), a.end(), want.begin()); }
// the four members exist for secp256k1 only
template <class C> concept has_btc = requires(W256 const& a, W256& o, wide_curve_point<C> const& q, hip::mask& m) {
  curve_group<C>::btc_pubkey_hash(q); curve_group<C>::xonly_tweak_add(a, a, m, m); curve_group<C>::taproot_tweak_pubkey(a, m, m); curve_group<C>::taproot_tweak_seckey(a, o, m);
};
static_assert(has_btc<curve_secp256k1> && !has_btc<curve_nist_p256>);
}  // namespace

TEST(Btc, HashKnownAnswers) {
  const hip::messages abc(std::vector<std::string>(default_lanes, std::string("abc")));
  EXPECT_TRUE(same(hip::ripemd160(abc).get(0), "8eb208f7e05d987a9b044a8e98c6b087f15a0bfc"_hex));
  EXPECT_TRUE(same(hip::ripemd160(abc).get(default_lanes - 1), "8eb208f7e05d987a9b044a8e98c6b087f15a0bfc"_hex));
  const hip::messages empty(std::vector<std::string>(default_lanes, std::string()));
  EXPECT_TRUE(same(hip::hash160(empty).get(0), "b472a266d0bd89c13706a4132ccfb16f7c3b9fcb"_hex));
  // SHA256(SHA256("abc")), and the same from two single hashes
  const W256 dd = hip::sha256d(abc);
  EXPECT_TRUE(dd.get(0) == bn("4f8b42c22dd3729b519ba6f68d2da7cc5b2d606d05daed5ad5128cc03e6c6358"_hex));
  // the P2PKH hash of secret key 1, both encodings
  const auto g = CG::scalar_mult_base_affine(W256{bignum_256::from(1)});
  EXPECT_TRUE(same(CG::btc_pubkey_hash(g).get(0), "751e76e8199196d454941c45d1b3a323f1433bd6"_hex));
  EXPECT_TRUE(same(CG::btc_pubkey_hash(g, false).get(0), "91b24bf9f5288532960ac687abb035127b1d28a5"_hex));
}

TEST(Btc, Bip341WalletVector) {
  const W256 px{bn("d6889cb081036e0faefa3a35157ad71086b123b2b144b649798b494c300a961d"_hex)};
  const W256 t{bn("b86e7be8f39bab32a6f2c0443abbc210f0edac0e2c53d501b36b64437d9c6c70"_hex)};
  const bignum_256 want = bn("53a1f6e454df1aa2776a2814a721372d6258050de330b3c6d10ee8f4e0dda343"_hex);
  hip::mask parity, ok;
  EXPECT_TRUE(CG::taproot_tweak_pubkey(px, parity, ok).get(0) == want && parity.get(0) && ok.get(0));
  EXPECT_TRUE(CG::xonly_tweak_add(px, t, parity, ok).get(0) == want && parity.get(0) && ok.get(0));
  EXPECT_TRUE(CG::xonly_tweak_add(px, W256{bignum_256::from(0)}, parity, ok).get(0) == px.get(0) && !parity.get(0) && ok.get(0));     // t = 0: Q = P
  EXPECT_TRUE(CG::taproot_tweak_pubkey(W256{bignum_256::from(5)}, parity, ok).get(0) == bignum_256::from(0) && !ok.get(0));           // x = 5 does not lift
}

TEST(Btc, KeyPathSpend) {
  const size_t n = 300;
  const W256 d(n, [](size_t i, size_t) { bignum_256 b; b.limbs = {0x9e3779b97f4a7c15ull * (i + 1), i * 77, ~i, 0x0123456789abcdefull ^ (i << 20)}; return b; });
  const W256 root(n, [](size_t i, size_t) { bignum_256 b; b.limbs = {i, ~i * 3, i << 40, 0xfedcba9876543210ull + i}; return b; });
  W256 px, spx; hip::mask ok, parity, qok, sok;
  const W256 tweaked = CG::taproot_tweak_seckey(d, px, ok, &root);
  EXPECT_TRUE(all(ok));
  const W256 qx = CG::taproot_tweak_pubkey(px, parity, qok, &root);
  EXPECT_TRUE(all(qok));
  std::vector<uint8_t> records(n * 32);
  for (size_t i = 0; i < records.size(); ++i) records[i] = (uint8_t)(i * 131 + (i >> 8));
  const hip::messages m(records.data(), n, 32, 32);
  const auto sig = CG::schnorr_sign(tweaked, m, spx, sok);
  EXPECT_TRUE(all(sok));
  EXPECT_TRUE(spx.get(0) == qx.get(0) && spx.get(n - 1) == qx.get(n - 1));
  EXPECT_TRUE(all(CG::schnorr_verify(qx, m, sig.first, sig.second)));
  // a key out of range is refused with zero outputs
  const W256 none = CG::taproot_tweak_seckey(W256{bignum_256::from(0)}, px, ok);
  EXPECT_TRUE(!ok.get(0) && none.get(0) == bignum_256::from(0) && px.get(0) == bignum_256::from(0));
}

int main() { return mini::run_all(); }
