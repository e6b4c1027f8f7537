// btc_tree_tests.cpp -- Bitcoin's hashes with one length per message, Merkle roots and BIP-341 script paths through the C++ host API (hip::sha256 / sha256d /
// hash160 / ripemd160 with hip::lengths, curve_group<curve_secp256k1>::btc_merkle_root / tapleaf_hash / taproot_merkle_path): the values of
// tests/golden/btc_tree_vectors.json.  Built and run by tests/test_cpp_btc_tree.py; the harness is mini_test.h.
#include <ecsimd/ecsimd.h>
#include "mini_test.h"

using namespace ecsimd;
using namespace ecsimd::literals;

namespace {
using W256 = wide_bignum<bignum_256>;
using CG = curve_group<curve_secp256k1>;
template <size_t N> bignum_256 bn(std::array<uint8_t, N> const& be) { return bn_from_bytes_BE<bignum_256>(be); }
template <size_t N> bignum_256 bn_reversed(std::array<uint8_t, N> be) { std::reverse(be.begin(), be.end()); return bn_from_bytes_BE<bignum_256>(be); }
template <size_t N> std::string str(std::array<uint8_t, N> const& b) { return std::string(b.begin(), b.end()); }
template <size_t N> bool same(hip::digests20::address const& a, std::array<uint8_t, N> const& want) { return N == 20 && std::equal(a.begin(), a.end(), want.begin()); }
// the three members exist for secp256k1 only
template <class C> concept has_trees = requires(W256 const& a, hip::messages const& m, hip::mask& ok) {
  curve_group<C>::btc_merkle_root(a, std::vector<uint64_t>{}); curve_group<C>::tapleaf_hash(m); curve_group<C>::taproot_merkle_path(a, m, 0u, ok);
};
static_assert(has_trees<curve_secp256k1> && !has_trees<curve_nist_p256>);
}  // namespace

TEST(BtcTree, OneLengthPerMessage) {
  // "abc", the empty message and the 56 bytes of FIPS 180-4's second example in one call
  const auto ml = hip::ragged({"abc", "", "abcdbcdecdefdefgefghfghighijhijkijkljklmklmnlmnomnopnopq"});
  const W256 e = hip::sha256(ml.first, ml.second);
  EXPECT_TRUE(e.get(0) == bn("ba7816bf8f01cfea414140de5dae2223b00361a396177a9cb410ff61f20015ad"_hex));
  EXPECT_TRUE(e.get(1) == bn("e3b0c44298fc1c149afbf4c8996fb92427ae41e4649b934ca495991b7852b855"_hex));
  EXPECT_TRUE(e.get(2) == bn("248d6a61d20638b8e5c026930c3e6039a33ce45964ff2167f6ecedd419db06c1"_hex));
  EXPECT_TRUE(hip::sha256d(ml.first, ml.second).get(0) == bn("4f8b42c22dd3729b519ba6f68d2da7cc5b2d606d05daed5ad5128cc03e6c6358"_hex));
  EXPECT_TRUE(same(hip::ripemd160(ml.first, ml.second).get(0), "8eb208f7e05d987a9b044a8e98c6b087f15a0bfc"_hex));
  EXPECT_TRUE(same(hip::ripemd160(ml.first, ml.second).get(2), "12a053384a9c0c88e405a06c27dcf49ada62eb2b"_hex));
  EXPECT_TRUE(same(hip::hash160(ml.first, ml.second).get(1), "b472a266d0bd89c13706a4132ccfb16f7c3b9fcb"_hex));
}

TEST(BtcTree, Block170) {
  const bignum_256 a = bn_reversed("b1fea52486ce0c62bb442b530a3f0132b826c74e473d1f2c220bfa78111c5082"_hex);
  const bignum_256 b = bn_reversed("f4184fc596403b9d638783cf57adfe4c75c605f6356fbc91338530e9831e9e16"_hex);
  const bignum_256 root = bn_reversed("7dac2c5666815c17a3b36427de37bb9d2e2c5ccec3f8633eb91a4205cb4c10ff"_hex);
  // the block; [a, b, b] and [a, b, b, b]: one root (CVE-2012-2459), told apart by the flag; a tree of one leaf is the leaf
  const std::vector<bignum_256> leaves = {a, b, a, b, b, a, b, b, b, b};
  const W256 wl(leaves.size(), [&](size_t i, size_t) { return leaves[i]; });
  hip::mask mutated;
  const W256 roots = CG::btc_merkle_root(wl, {2, 3, 4, 1}, &mutated);
  EXPECT_TRUE(roots.get(0) == root && roots.get(1) == roots.get(2) && !(roots.get(1) == root) && roots.get(3) == b);
  EXPECT_TRUE(!mutated.get(0) && !mutated.get(1) && mutated.get(2) && !mutated.get(3));
  EXPECT_TRUE(CG::btc_merkle_root(wl, {2, 3, 4, 1}).get(0) == root);
}

TEST(BtcTree, Bip341ScriptPath) {
  const auto script = "20d85a959b0290bf19bb89ed43c916be835475d013da4b362117393e25a48229b8ac"_hex;
  const W256 px(1, bn("187791b6f712a8ea41c8ecdd0ee77fab3e85263b37e1ec18a3651926b3a6cf27"_hex));                     // one lane, as the one script
  const bignum_256 leaf_hash = bn("5b75adecf53548f3ec6ad7d78383bf84cc57b55a3127c72b9a2481752dd88b21"_hex);
  const hip::messages scripts(std::vector<std::string>{str(script)});
  const W256 leaf = CG::tapleaf_hash(scripts);
  EXPECT_TRUE(leaf.get(0) == leaf_hash);
  const auto rl = hip::ragged({str(script) + "padding behind the script"});
  // ragged rounds the row up to a multiple of 4: without lens the whole row is the script, with them the string alone, and neither is the vector's script
  const hip::lengths whole_row(std::vector<uint32_t>{(uint32_t)rl.first.msg_bytes()});
  EXPECT_TRUE(CG::tapleaf_hash(rl.first, &whole_row).get(0) == CG::tapleaf_hash(rl.first).get(0));
  EXPECT_TRUE(!(CG::tapleaf_hash(rl.first, &rl.second).get(0) == CG::tapleaf_hash(rl.first).get(0)) && !(CG::tapleaf_hash(rl.first, &rl.second).get(0) == leaf_hash));
  const hip::lengths only_the_script(std::vector<uint32_t>{(uint32_t)script.size()});
  EXPECT_TRUE(CG::tapleaf_hash(rl.first, &only_the_script).get(0) == leaf_hash);
  // depth 0: the leaf hash is the merkle root; the output key and its parity are the vector's
  const hip::messages no_path(std::vector<std::string>{std::string(32, '\0')});
  hip::mask ok, parity, tok;
  const W256 root = CG::taproot_merkle_path(leaf, no_path, 0, ok);
  EXPECT_TRUE(root.get(0) == leaf_hash && ok.get(0));
  EXPECT_TRUE(CG::taproot_tweak_pubkey(px, parity, tok, &root).get(0) == bn("147c9c57132f6e7ecddba9800bb0c4449251c92a1e60371ee77557b6620f3ea3"_hex) && parity.get(0) && tok.get(0));
  // depth 1 with the leaf as its own sibling is H_TapBranch(leaf || leaf) whichever way the pair is ordered; depth 129 is refused
  std::array<uint8_t, 32> leaf_bytes = "5b75adecf53548f3ec6ad7d78383bf84cc57b55a3127c72b9a2481752dd88b21"_hex;
  const hip::messages sibling(std::vector<std::string>{str(leaf_bytes)});
  const std::vector<uint8_t> one = {1};
  EXPECT_TRUE(CG::taproot_merkle_path(leaf, sibling, 0, ok, &one).get(0) == CG::taproot_merkle_path(leaf, sibling, 1, ok).get(0) && ok.get(0));
  EXPECT_TRUE(!(CG::taproot_merkle_path(leaf, sibling, 1, ok).get(0) == leaf_hash));
  EXPECT_TRUE(CG::taproot_merkle_path(leaf, sibling, 129, ok).get(0) == bignum_256::from(0) && !ok.get(0));
}

int main() { return mini::run_all(); }
