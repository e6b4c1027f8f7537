// ecsimd/curve_group.h -- curve_group<Curve>: the co-Z formulas and the ladder (reference curve_group.h:20-252).
// Same static member names and parameter conventions: reference parameters that the reference
// updates in place (DBLU's P, ZADDU's P, ZDAU's Q, TRPLU's P) are updated in place here too.
#ifndef ECSIMD_CURVE_GROUP_H
#define ECSIMD_CURVE_GROUP_H
#include <ecsimd/device_group.h>
#include <ecsimd/curve_secp256k1.h>
#include <ecsimd/jacobian_curve_point.h>
#include <ecsimd/keccak256.h>
#include <ecsimd/hash160.h>
#include <ecsimd/sha256.h>
#include <ecsimd/sha512.h>
#include <ecsimd_schnorr_batch.h>
#include <optional>
#include <type_traits>

namespace ecsimd {
template <class Curve>
struct curve_group {
  using WBN = curve_wide_bn_t<Curve>;
  using BN = typename WBN::value_type;
  using WMBN = wide_mgry_bignum<WBN, typename Curve::P>;
  using gfp = GFp<WBN, typename Curve::P>;
  using WCP = wide_curve_point<Curve>;
  using WJCP = wide_jacobian_curve_point<Curve>;
  static int curve_id() { return WJCP::curve_id(); }
  // what this curve's id can do beyond the reference's layers (ecsimd_hip_curve_capabilities): decided once, at registration
  static bool can(int capability) { static const int caps = [] { int c = 0; hip::check(ecsimd_hip_curve_capabilities(curve_id(), &c), "ecsimd_hip_curve_capabilities"); return c; }(); return (caps & capability) != 0; }

  static BN Am() { return curve_constant(8); }      // curve_group.h:32
  static BN Bm() { return curve_constant(9); }      // curve_group.h:31
  static BN curve_constant(int which) { BN r; hip::check(ecsimd_hip_get_constant(curve_id(), which, r.limbs.data()), "ecsimd_hip_get_constant"); return r; }
  static WCP WG(size_t lanes = default_lanes) { return WCP{WBN(lanes, Curve::Gx::value), WBN(lanes, Curve::Gy::value)}; }   // :35-37
  static WJCP WJG(size_t lanes = default_lanes) { return WJCP::from_affine(WG(lanes)); }                                     // :39-41

  static std::optional<WBN> compute_y(WBN const& x) {                        // :52-58 (all lanes or nothing, like the reference)
    hip::mask ok; WBN y = compute_y_lanes(x, ok); if (!all(ok)) return {}; return {y};
  }
  static WBN compute_y_lanes(WBN const& x, hip::mask& ok) {                  // per-lane validity; y^2 = x^3 + a x + b for either curve
    auto y = WBN::uninitialized(x.size()); ok = hip::mask(x.size());
    hip::check(ecsimd_hip_compute_y(hip::context(), curve_id(), x.data(), y.data(), ok.data(), x.size()), "ecsimd_hip_compute_y"); return y;
  }

  static WJCP DBLU(WJCP& P) {                                                // :64-87
    P.unshare(); WJCP r = fresh_xy(P.size());                               // co-Z: r and the rewritten P share ONE Z array, written once
    hip::check(ecsimd_hip_dblu(hip::context(), curve_id(), px(P), py(P), pz(P), px(r), py(r), pz(P), P.size()), "ecsimd_hip_dblu"); r.z() = P.z(); return r;
  }
  static WJCP ZADDU(WJCP& P, WJCP const& O) {                                // :91-116
    same_length(P.size(), O.size(), "ZADDU");
    P.unshare(); WJCP r = fresh_xy(P.size());
    hip::check(ecsimd_hip_zaddu(hip::context(), curve_id(), px(P), py(P), pz(P), px(O), py(O), pz(O), px(r), py(r), pz(P), P.size()), "ecsimd_hip_zaddu"); r.z() = P.z(); return r;
  }
  static WJCP ZDAU(WJCP const& P, WJCP& Q) {                                 // :120-153
    same_length(P.size(), Q.size(), "ZDAU");
    Q.unshare(); WJCP r = fresh_xy(P.size());
    hip::check(ecsimd_hip_zdau(hip::context(), curve_id(), px(P), py(P), pz(P), px(Q), py(Q), pz(Q), px(r), py(r), pz(Q), P.size()), "ecsimd_hip_zdau"); r.z() = Q.z(); return r;
  }
  static WJCP ADD_Z2_1(WJCP const& A, WJCP const& B) {                       // :155-179 (B.z must be mgry(1))
    same_length(A.size(), B.size(), "ADD_Z2_1");
    WJCP r = fresh(A.size());
    hip::check(ecsimd_hip_add_z2_1(hip::context(), curve_id(), px(A), py(A), pz(A), px(B), py(B), px(r), py(r), pz(r), A.size()), "ecsimd_hip_add_z2_1"); return r;
  }
  static WJCP TRPLU(WJCP& P) {                                               // :183-186
    P.unshare(); WJCP r = fresh_xy(P.size());
    hip::check(ecsimd_hip_trplu(hip::context(), curve_id(), px(P), py(P), pz(P), px(r), py(r), pz(P), P.size()), "ecsimd_hip_trplu"); r.z() = P.z(); return r;
  }
  // k[i] * P[i], P.z must be mgry(1) (:189-218).  One kernel: the whole ladder stays in registers.
  static WJCP scalar_mult(WBN const& x, WJCP P) {
    same_length(x.size(), P.size(), "scalar_mult");
    WJCP r = fresh(P.size());
    hip::check(ecsimd_hip_scalar_mult(hip::context(), curve_id(), x.data(), px(P), py(P), px(r), py(r), pz(r), P.size(), ECSIMD_HIP_BASE_MGRY | ECSIMD_HIP_OUT_JACOBIAN), "ecsimd_hip_scalar_mult"); return r;
  }
  // one scalar for every lane (:221-251)
  static WJCP scalar_mult_1s(BN const& x, WJCP P) {
    WJCP r = fresh(P.size());
    hip::check(ecsimd_hip_scalar_mult_1s(hip::context(), curve_id(), x.limbs.data(), px(P), py(P), px(r), py(r), pz(r), P.size(), ECSIMD_HIP_BASE_MGRY | ECSIMD_HIP_OUT_JACOBIAN), "ecsimd_hip_scalar_mult_1s"); return r;
  }

  // ---- extensions (not in the reference): affine-level entry points over the faster algorithms of the C ABI.
  // Same points as to_affine() of the ladder's result for every scalar where the ladder is non-degenerate.
  // (The ladder fallback returns the LADDER's point, not k P, at the ladder's degenerate scalars: n - 1 and k | 1 = 2^j mod n for bitlen(n) <= j <= 256.)
  // k[i] * P[i], P affine classical -> affine classical.  windowed: per-element tables of 8 multiples of P + signed 4-bit
  // windows (ECSIMD_HIP_ALG_WINDOWED); otherwise the reference ladder followed by one simultaneous inversion.  A curve registered at run time has the
  // tables when it names a prime order N >= 2^255 (ECSIMD_HIP_CURVE_WINDOW_VARIABLE_BASE); without it the same points come from the ladder.
  static WCP scalar_mult_affine(WBN const& x, WCP const& P, bool windowed = true) {
    same_length(x.size(), P.size(), "scalar_mult_affine");
    WCP r{WBN::uninitialized(P.size()), WBN::uninitialized(P.size())};
    const bool tables = windowed && can(ECSIMD_HIP_CURVE_WINDOW_VARIABLE_BASE);
    hip::check(ecsimd_hip_scalar_mult(hip::context(), curve_id(), x.data(), P.x().data(), P.y().data(), r.x().data(), r.y().data(), nullptr, P.size(),
                                      ECSIMD_HIP_BASE_CLASSICAL | ECSIMD_HIP_OUT_AFFINE | (tables ? ECSIMD_HIP_ALG_WINDOWED : 0)), "ecsimd_hip_scalar_mult");
    return r;
  }
  // A + B for every input, unlike ADD_Z2_1: A = B, A = -B (Z = 0 comes back), A at infinity (Z = 0); B.z must be mgry(1).
  static WJCP add_mixed_complete(WJCP const& A, WJCP const& B) {
    same_length(A.size(), B.size(), "add_mixed_complete");
    WJCP r = fresh(A.size());
    hip::check(ecsimd_hip_add_mixed_complete(hip::context(), curve_id(), px(A), py(A), pz(A), px(B), py(B), px(r), py(r), pz(r), A.size()), "ecsimd_hip_add_mixed_complete"); return r;
  }
  // k[i] * G through the 20-bit window table of odd multiples in device memory (12 mixed additions), affine classical.  A curve registered at run time
  // (one that names its order N) has the signed 7-bit table of its generator in LDS instead (36 mixed additions).
  static WCP scalar_mult_base_affine(WBN const& x) {
    WCP r{WBN::uninitialized(x.size()), WBN::uninitialized(x.size())};
    const int alg = !can(ECSIMD_HIP_CURVE_COMB) ? 0 : curve_id() >= ECSIMD_HIP_FIRST_REGISTERED_CURVE ? ECSIMD_HIP_ALG_WINDOWED_SIGNED : ECSIMD_HIP_ALG_WINDOWED_BIG;   // (no order, or n < 2^255: no table, the ladder)
    hip::check(ecsimd_hip_scalar_mult_base(hip::context(), curve_id(), x.data(), r.x().data(), r.y().data(), nullptr, x.size(),
                                           ECSIMD_HIP_OUT_AFFINE | alg), "ecsimd_hip_scalar_mult_base");
    return r;
  }
  // k[i] * P[i] for SECRET scalars (ECDH): the per-element window tables with ECSIMD_HIP_ALG_CONSTANT_TIME -- every entry of the lane's
  // table read in every window, kept under lane masks; 1.45 x (P-256) / 1.74 x (secp256k1) the ladder.  Affine classical in and out.
  static WCP scalar_mult_affine_secret(WBN const& x, WCP const& P) {
    same_length(x.size(), P.size(), "scalar_mult_affine_secret");
    WCP r{WBN::uninitialized(P.size()), WBN::uninitialized(P.size())};
    const int alg = can(ECSIMD_HIP_CURVE_WINDOW_VARIABLE_BASE) ? (ECSIMD_HIP_ALG_WINDOWED | ECSIMD_HIP_ALG_CONSTANT_TIME) : 0;      // (without the tables: the ladder, constant-time as it is)
    hip::check(ecsimd_hip_scalar_mult(hip::context(), curve_id(), x.data(), P.x().data(), P.y().data(), r.x().data(), r.y().data(), nullptr, P.size(),
                                      ECSIMD_HIP_BASE_CLASSICAL | ECSIMD_HIP_OUT_AFFINE | alg), "ecsimd_hip_scalar_mult");
    return r;
  }
  // k[i] * G for SECRET scalars (key generation, ECDSA nonces): an LDS comb with ECSIMD_HIP_ALG_CONSTANT_TIME -- every table entry of a
  // window read, the wanted one kept under lane masks, no address or branch formed from the scalar; 6.7 x the ladder on G.  Affine classical.
  static WCP scalar_mult_base_affine_secret(WBN const& x) {
    WCP r{WBN::uninitialized(x.size()), WBN::uninitialized(x.size())};
    const int alg = can(ECSIMD_HIP_CURVE_COMB) ? (ECSIMD_HIP_ALG_WINDOWED | ECSIMD_HIP_ALG_CONSTANT_TIME) : 0;      // (without the comb: the ladder, constant-time as it is; its point, not k G, at its degenerate scalars)
    hip::check(ecsimd_hip_scalar_mult_base(hip::context(), curve_id(), x.data(), r.x().data(), r.y().data(), nullptr, x.size(),
                                           ECSIMD_HIP_OUT_AFFINE | alg), "ecsimd_hip_scalar_mult_base");
    return r;
  }
  // u1[i] * G + u2[i] * Q[i] (the ECDSA-verification shape), affine classical; finite[i] is false where the sum
  // is the point at infinity (coordinates (0, 0)).
  static WCP double_scalar_mult(WBN const& u1, WBN const& u2, WCP const& Q, hip::mask& finite) {
    same_length(u1.size(), Q.size(), "double_scalar_mult"); same_length(u2.size(), Q.size(), "double_scalar_mult");
    WCP r{WBN::uninitialized(Q.size()), WBN::uninitialized(Q.size())};
    finite = hip::mask(Q.size());
    hip::check(ecsimd_hip_double_scalar_mult(hip::context(), curve_id(), u1.data(), u2.data(), Q.x().data(), Q.y().data(), r.x().data(), r.y().data(),
                                             finite.data(), Q.size()), "ecsimd_hip_double_scalar_mult");
    return r;
  }
  // ECDSA's acceptance test for precomputed u1 = e/s, u2 = r/s (mod n): lane i is set iff u1*G + u2*Q is finite and its x mod n == r.
  static hip::mask ecdsa_verify_rx(WBN const& u1, WBN const& u2, WCP const& Q, WBN const& r) {
    same_length(u1.size(), Q.size(), "ecdsa_verify_rx"); same_length(u2.size(), Q.size(), "ecdsa_verify_rx"); same_length(r.size(), Q.size(), "ecdsa_verify_rx");
    hip::mask ok(Q.size());
    hip::check(ecsimd_hip_ecdsa_verify_rx(hip::context(), curve_id(), u1.data(), u2.data(), Q.x().data(), Q.y().data(), r.data(), ok.data(), Q.size()), "ecsimd_hip_ecdsa_verify_rx");
    return ok;
  }
  // The whole ECDSA verification (SEC 1 v2 4.1.4): e = the digest as an integer (any 256-bit value), (r, s) the signature, Q the public key.
  // Lane i is set iff 1 <= r, s < n, Q is a valid public key and x((e/s) G + (r/s) Q) mod n == r.  The arithmetic modulo the group order
  // runs on the device (the field layer on the order's field id; GFp<WBN, p256_order> / GFp<WBN, secp256k1_order> is the same arithmetic).
  static hip::mask ecdsa_verify(WBN const& e, WBN const& r, WBN const& s, WCP const& Q) {
    same_length(e.size(), Q.size(), "ecdsa_verify"); same_length(r.size(), Q.size(), "ecdsa_verify"); same_length(s.size(), Q.size(), "ecdsa_verify");
    hip::mask ok(Q.size());
    hip::check(ecsimd_hip_ecdsa_verify(hip::context(), curve_id(), e.data(), r.data(), s.data(), Q.x().data(), Q.y().data(), ok.data(), Q.size()), "ecsimd_hip_ecdsa_verify");
    return ok;
  }
  // ECDSA signing (SEC 1 v2 4.1.3): digests e, private keys d, the CALLER's nonces k (RFC 6979 or a DRBG).  Returns (r, s); ok[i] is false -- and
  // r = s = 0 -- where d or k is not in [1, n) or r or s came out zero.  k G runs on the constant-time comb; no branch or address depends on d or k.
  static std::pair<WBN, WBN> ecdsa_sign(WBN const& e, WBN const& d, WBN const& k, hip::mask& ok) {
    same_length(e.size(), d.size(), "ecdsa_sign"); same_length(k.size(), d.size(), "ecdsa_sign");
    auto r = WBN::uninitialized(d.size()), s = WBN::uninitialized(d.size());
    ok = hip::mask(d.size());
    hip::check(ecsimd_hip_ecdsa_sign(hip::context(), curve_id(), e.data(), d.data(), k.data(), r.data(), s.data(), ok.data(), d.size()), "ecsimd_hip_ecdsa_sign");
    return {r, s};
  }
  // Public-key recovery (SEC 1 v2 4.1.6): the key Q behind each signature (r, s) of the digest e, given the recovery id v -- one byte per lane in a hip::mask's
  // storage: bit 0 = the parity of y(k G), bit 1 = x(k G) >= n, as ecdsa_sign_recoverable returns it.  ok[i] is false -- and Q[i] = (0, 0) -- where v > 3, r or s
  // is not in [1, n), r + (v >> 1) n is not the x of a curve point, or the recovered point is infinite.  Public data only.
  static WCP ecdsa_recover(WBN const& e, WBN const& r, WBN const& s, hip::mask const& v, hip::mask& ok) {
    same_length(r.size(), e.size(), "ecdsa_recover"); same_length(s.size(), e.size(), "ecdsa_recover"); same_length(v.size(), e.size(), "ecdsa_recover");
    WCP q{WBN::uninitialized(e.size()), WBN::uninitialized(e.size())};
    ok = hip::mask(e.size());
    hip::check(ecsimd_hip_ecdsa_recover(hip::context(), curve_id(), e.data(), r.data(), s.data(), v.data(), q.x().data(), q.y().data(), ok.data(), e.size()), "ecsimd_hip_ecdsa_recover");
    return q;
  }
  // ecdsa_sign that also returns the recovery id v (0 where ok[i] is false); low_s: s > n / 2 is returned as n - s and bit 0 of v flipped.
  static std::pair<WBN, WBN> ecdsa_sign_recoverable(WBN const& e, WBN const& d, WBN const& k, hip::mask& v, hip::mask& ok, bool low_s = false) {
    same_length(e.size(), d.size(), "ecdsa_sign_recoverable"); same_length(k.size(), d.size(), "ecdsa_sign_recoverable");
    auto r = WBN::uninitialized(d.size()), s = WBN::uninitialized(d.size());
    v = hip::mask(d.size()); ok = hip::mask(d.size());
    hip::check(ecsimd_hip_ecdsa_sign_recoverable(hip::context(), curve_id(), e.data(), d.data(), k.data(), r.data(), s.data(), v.data(), ok.data(), d.size(),
                                                 low_s ? ECSIMD_HIP_ECDSA_LOW_S : 0), "ecsimd_hip_ecdsa_sign_recoverable");
    return {r, s};
  }
  // Deterministic signing (RFC 6979 with HMAC-SHA-256): ecdsa_sign_recoverable with the nonce of (e, d) made on the device and wiped before the call returns;
  // the caller never sees it.  Bit for bit the chain rfc6979_nonce -> ecdsa_sign_recoverable.  Curves whose order is at least 2^255.
  static std::pair<WBN, WBN> ecdsa_sign_deterministic(WBN const& e, WBN const& d, hip::mask& v, hip::mask& ok, bool low_s = false) {
    same_length(e.size(), d.size(), "ecdsa_sign_deterministic");
    auto r = WBN::uninitialized(d.size()), s = WBN::uninitialized(d.size());
    v = hip::mask(d.size()); ok = hip::mask(d.size());
    hip::check(ecsimd_hip_ecdsa_sign_deterministic(hip::context(), curve_id(), e.data(), d.data(), r.data(), s.data(), v.data(), ok.data(), d.size(),
                                                   low_s ? ECSIMD_HIP_ECDSA_LOW_S : 0), "ecsimd_hip_ecdsa_sign_deterministic");
    return {r, s};
  }
  // the nonce by itself (a SECRET: for callers that sign elsewhere); ok[i] is false and k[i] = 0 where d is not in [1, n)
  static WBN rfc6979_nonce(WBN const& e, WBN const& d, hip::mask& ok) {
    same_length(e.size(), d.size(), "rfc6979_nonce");
    auto k = WBN::uninitialized(d.size()); ok = hip::mask(d.size());
    hip::check(ecsimd_hip_rfc6979_nonce(hip::context(), curve_id(), e.data(), d.data(), k.data(), ok.data(), d.size()), "ecsimd_hip_rfc6979_nonce");
    return k;
  }
  // ---- BIP-340 Schnorr signatures: defined for secp256k1 only, so these two members exist in curve_group<curve_secp256k1> and nowhere else.
  // Verification of the signatures (r, s) of the messages m (hip::messages: equal lengths, any stride) under the x-only public keys px.  Public data only.
  static hip::mask schnorr_verify(WBN const& px, hip::messages const& m, WBN const& r, WBN const& s) requires std::is_same_v<Curve, curve_secp256k1> {
    same_length(px.size(), m.size(), "schnorr_verify"); same_length(r.size(), m.size(), "schnorr_verify"); same_length(s.size(), m.size(), "schnorr_verify");
    hip::mask ok(m.size());
    hip::check(ecsimd_hip_schnorr_verify(hip::context(), px.data(), m.data(), m.msg_bytes(), m.stride_bytes(), r.data(), s.data(), ok.data(), m.size()), "ecsimd_hip_schnorr_verify");
    return ok;
  }
  // ONE verdict for the whole batch: true iff every signature is valid (ecsimd_schnorr_batch.h: a batch with an invalid one passes with probability at most
  // 2^-127 on the MSM route; an empty batch is accepted).  route: ECSIMD_SCHNORR_BATCH_AUTO, _MSM or _LANES.  Waits for the stream to read the byte;
  // hip::schnorr_verify_batch (ecsimd/schnorr_batch.h) leaves it on the device.  Which lane is at fault is schnorr_verify's to say.
  static bool schnorr_verify_batch(WBN const& px, hip::messages const& m, WBN const& r, WBN const& s, int route = ECSIMD_SCHNORR_BATCH_AUTO) requires std::is_same_v<Curve, curve_secp256k1> {
    same_length(px.size(), m.size(), "schnorr_verify_batch"); same_length(r.size(), m.size(), "schnorr_verify_batch"); same_length(s.size(), m.size(), "schnorr_verify_batch");
    hip::mask ok(1);
    hip::check(ecsimd_schnorr_verify_batch(hip::context(), px.data(), m.data(), m.msg_bytes(), m.stride_bytes(), r.data(), s.data(), ok.data(), m.size(), route), "ecsimd_schnorr_verify_batch");
    return ok.get(0);
  }
  // Default signing with the SECRET keys d and the auxiliary randomness aux (nullptr: 32 zero bytes): returns (r, s), px = the x-only public keys.  ok[i] is
  // false -- and r = s = px = 0 -- where d is not in [1, n).  Both products run on the constant-time comb; no branch or address depends on d, aux or the nonce.
  static std::pair<WBN, WBN> schnorr_sign(WBN const& d, hip::messages const& m, WBN& px, hip::mask& ok, WBN const* aux = nullptr) requires std::is_same_v<Curve, curve_secp256k1> {
    same_length(d.size(), m.size(), "schnorr_sign"); if (aux) same_length(aux->size(), m.size(), "schnorr_sign");
    auto r = WBN::uninitialized(d.size()), s = WBN::uninitialized(d.size());
    px = WBN::uninitialized(d.size()); ok = hip::mask(d.size());
    hip::check(ecsimd_hip_schnorr_sign(hip::context(), d.data(), m.data(), m.msg_bytes(), m.stride_bytes(), aux ? aux->data() : nullptr, px.data(), r.data(), s.data(), ok.data(),
                                       d.size()), "ecsimd_hip_schnorr_sign");
    return {r, s};
  }
  // ---- Ethereum: secp256k1 only, like the Schnorr members.  Public data only.
  // The addresses of the public keys q: the last 20 bytes of Keccak-256 over each key's 64 big-endian bytes.  No validation: the 64 bytes are hashed as given.
  static hip::addresses eth_address(WCP const& q) requires std::is_same_v<Curve, curve_secp256k1> {
    hip::addresses a(q.x().size());
    hip::check(ecsimd_hip_eth_address(hip::context(), q.x().data(), q.y().data(), a.data(), a.size()), "ecsimd_hip_eth_address");
    return a;
  }
  // ecrecover: the sender address behind each signature (r, s) of the digest e (hip::keccak256 of the signing bytes), v = 0, 1, 27 or 28 in a hip::mask's storage.
  // ok[i] is false -- and the address 20 zero bytes -- where v is anything else, where ecdsa_recover refuses the signature, and, with
  // ECSIMD_HIP_ETH_REQUIRE_LOW_S in flags, where s > n / 2.  The recovered key stays on the device and is not returned.
  static hip::addresses eth_recover(WBN const& e, WBN const& r, WBN const& s, hip::mask const& v, hip::mask& ok, int flags = 0) requires std::is_same_v<Curve, curve_secp256k1> {
    same_length(r.size(), e.size(), "eth_recover"); same_length(s.size(), e.size(), "eth_recover"); same_length(v.size(), e.size(), "eth_recover");
    hip::addresses a(e.size());
    ok = hip::mask(e.size());
    hip::check(ecsimd_hip_eth_recover(hip::context(), e.data(), r.data(), s.data(), v.data(), a.data(), nullptr, nullptr, ok.data(), e.size(), flags), "ecsimd_hip_eth_recover");
    return a;
  }
  // ---- Bitcoin: secp256k1 only, like the Schnorr and the Ethereum members.
  // HASH160 of the SEC1 encoding of the public keys q (33 bytes, or 65 with compressed = false): what a P2PKH / P2WPKH output holds.  No validation.  Public data.
  static hip::digests20 btc_pubkey_hash(WCP const& q, bool compressed = true) requires std::is_same_v<Curve, curve_secp256k1> {
    hip::digests20 h(q.x().size());
    hip::check(ecsimd_hip_btc_pubkey_hash(hip::context(), q.x().data(), q.y().data(), h.data(), h.size(), compressed ? 1 : 0), "ecsimd_hip_btc_pubkey_hash");
    return h;
  }
  // x(Q) for Q = lift_x(px) + t G; parity[i] = y(Q) & 1; ok[i] is false -- and x(Q) = 0 -- where px does not lift, t >= n or Q is infinite.  Public data.
  static WBN xonly_tweak_add(WBN const& px, WBN const& t, hip::mask& parity, hip::mask& ok) requires std::is_same_v<Curve, curve_secp256k1> {
    same_length(px.size(), t.size(), "xonly_tweak_add");
    auto qx = WBN::uninitialized(px.size()); parity = hip::mask(px.size()); ok = hip::mask(px.size());
    hip::check(ecsimd_hip_xonly_tweak_add(hip::context(), px.data(), t.data(), qx.data(), parity.data(), ok.data(), px.size()), "ecsimd_hip_xonly_tweak_add");
    return qx;
  }
  // BIP-341: the output key of the internal keys px, tweaked by H_TapTweak(px || merkle_root), or by H_TapTweak(px) with merkle_root = nullptr.  Public data.
  static WBN taproot_tweak_pubkey(WBN const& px, hip::mask& parity, hip::mask& ok, WBN const* merkle_root = nullptr) requires std::is_same_v<Curve, curve_secp256k1> {
    if (merkle_root) same_length(px.size(), merkle_root->size(), "taproot_tweak_pubkey");
    auto qx = WBN::uninitialized(px.size()); parity = hip::mask(px.size()); ok = hip::mask(px.size());
    hip::check(ecsimd_hip_taproot_tweak_pubkey(hip::context(), px.data(), merkle_root ? merkle_root->data() : nullptr, qx.data(), parity.data(), ok.data(), px.size()),
               "ecsimd_hip_taproot_tweak_pubkey");
    return qx;
  }
  // BIP-341: the SECRET key of that output key from the secret keys d, ready for schnorr_sign; px = x(d G), the internal keys.  ok[i] is false -- and both are
  // 0 -- where d is not in [1, n), the tweak is >= n or the sum is 0.  d G runs on the constant-time comb; no branch or address depends on d or the result.
  static WBN taproot_tweak_seckey(WBN const& d, WBN& px, hip::mask& ok, WBN const* merkle_root = nullptr) requires std::is_same_v<Curve, curve_secp256k1> {
    if (merkle_root) same_length(d.size(), merkle_root->size(), "taproot_tweak_seckey");
    auto out = WBN::uninitialized(d.size()); px = WBN::uninitialized(d.size()); ok = hip::mask(d.size());
    hip::check(ecsimd_hip_taproot_tweak_seckey(hip::context(), d.data(), merkle_root ? merkle_root->data() : nullptr, out.data(), px.data(), ok.data(), d.size()),
               "ecsimd_hip_taproot_tweak_seckey");
    return out;
  }
  // ---- Bitcoin's trees: Merkle roots of txids and BIP-341 script paths.  Public data.
  // The Merkle roots of counts.size() trees of txids (as hip::sha256d returns them), tree after tree in `leaves`; Bitcoin's rule.  mutated (optional): one flag
  // per tree, set where some level holds a real pair of equal nodes (CVE-2012-2459).
  static WBN btc_merkle_root(WBN const& leaves, std::vector<uint64_t> const& counts, hip::mask* mutated = nullptr) requires std::is_same_v<Curve, curve_secp256k1> {
    std::vector<uint64_t> offsets(counts.size() + 1, 0);
    for (size_t t = 0; t < counts.size(); ++t) offsets[t + 1] = offsets[t] + counts[t];
    same_length(leaves.size(), offsets.back(), "btc_merkle_root");
    auto roots = WBN::uninitialized(counts.size());
    if (mutated) *mutated = hip::mask(counts.size());
    hip::check(ecsimd_hip_btc_merkle_root(hip::context(), leaves.data(), offsets.data(), counts.size(), roots.data(), mutated ? mutated->data() : nullptr), "ecsimd_hip_btc_merkle_root");
    return roots;
  }
  // BIP-341: the leaf hashes H_TapLeaf(leaf_version || compact_size(len) || script) of the scripts (lens = nullptr: of one length).
  static WBN tapleaf_hash(hip::messages const& scripts, hip::lengths const* lens = nullptr, uint8_t leaf_version = 0xc0) requires std::is_same_v<Curve, curve_secp256k1> {
    if (lens) hip::same_rows(scripts, *lens);
    auto e = WBN::uninitialized(scripts.size());
    hip::check(ecsimd_hip_tapleaf_hash(hip::context(), scripts.data(), scripts.msg_bytes(), scripts.stride_bytes(), lens ? lens->data() : nullptr, nullptr, leaf_version, e.data(),
                                       scripts.size()), "ecsimd_hip_tapleaf_hash");
    return e;
  }
  // BIP-341: the merkle root each leaf hash reaches over the first `depth` nodes (32 bytes each, the leaf's sibling first) of its row of `path` -- or over
  // depths[i] of them; ok[i] is false, and the root 0, where a depth is above 128.  The root feeds taproot_tweak_pubkey.
  static WBN taproot_merkle_path(WBN const& leaf, hip::messages const& path, uint32_t depth, hip::mask& ok, std::vector<uint8_t> const* depths = nullptr)
      requires std::is_same_v<Curve, curve_secp256k1> {
    same_length(leaf.size(), path.size(), "taproot_merkle_path");
    hip::mask per_lane;
    if (depths) {
      same_length(leaf.size(), depths->size(), "taproot_merkle_path");
      per_lane = hip::mask(depths->size());
      if (!depths->empty()) hip::check(ecsimd_hip_memcpy_h2d(hip::context(), per_lane.data(), depths->data(), depths->size()), "h2d");
    }
    auto root = WBN::uninitialized(leaf.size()); ok = hip::mask(leaf.size());
    hip::check(ecsimd_hip_taproot_merkle_path(hip::context(), leaf.data(), path.data(), path.stride_bytes(), depths ? per_lane.data() : nullptr, depth, root.data(), ok.data(),
                                              leaf.size()), "ecsimd_hip_taproot_merkle_path");
    return root;
  }
  // ---- BIP-32 key derivation: secp256k1 only.  Keys and chain codes are the integers whose 32 big-endian bytes the BIP writes; an index >= 2^31 is hardened.
  // The master key and chain code of the SECRET seeds (16 .. 64 bytes each, one length); ok[i] is false -- and both are 0 -- where the key would be 0 or >= n.
  static WBN bip32_master(hip::messages const& seeds, WBN& c, hip::mask& ok) requires std::is_same_v<Curve, curve_secp256k1> {
    auto k = WBN::uninitialized(seeds.size()); c = WBN::uninitialized(seeds.size()); ok = hip::mask(seeds.size());
    hip::check(ecsimd_hip_bip32_master(hip::context(), seeds.data(), seeds.msg_bytes(), seeds.stride_bytes(), k.data(), c.data(), ok.data(), seeds.size()), "ecsimd_hip_bip32_master");
    return k;
  }
  // The master key and chain code of the SECRET BIP-39 sentences (equal lengths; one passphrase each, or one for all): hip::bip39_seed, then bip32_master on the
  // 64-byte seeds, which stay in device memory.
  static WBN bip39_master(hip::messages const& mnemonics, hip::messages const& passphrases, WBN& c, hip::mask& ok) requires std::is_same_v<Curve, curve_secp256k1> {
    const hip::derived_keys seeds = hip::bip39_seed(mnemonics, passphrases);
    auto k = WBN::uninitialized(seeds.size()); c = WBN::uninitialized(seeds.size()); ok = hip::mask(seeds.size());
    hip::check(ecsimd_hip_bip32_master(hip::context(), seeds.data(), 64, 64, k.data(), c.data(), ok.data(), seeds.size()), "ecsimd_hip_bip32_master");
    return k;
  }
  // CKDpriv of the SECRET nodes (k, c) at one index for every lane, or at index[i]; c_child is written, the child key returned.  ok[i] is false -- and both are
  // 0 -- where k is not in [1, n).  flags: ECSIMD_HIP_BIP32_ALL_HARDENED, the promise that every index is hardened (no point multiplication).  A hardened index for
  // every lane takes that route by itself.  k G runs on the constant-time comb; no branch or address depends on k, c or the results.
  static WBN bip32_ckd_priv(WBN const& k, WBN const& c, uint32_t index, WBN& c_child, hip::mask& ok, int flags = 0) requires std::is_same_v<Curve, curve_secp256k1> {
    return bip32_ckd_priv_impl(k, c, nullptr, index, c_child, ok, flags);
  }
  static WBN bip32_ckd_priv(WBN const& k, WBN const& c, hip::indices const& index, WBN& c_child, hip::mask& ok, int flags = 0) requires std::is_same_v<Curve, curve_secp256k1> {
    same_length(k.size(), index.size(), "bip32_ckd_priv");
    return bip32_ckd_priv_impl(k, c, index.data(), 0, c_child, ok, flags);
  }
  // CKDpub of the public nodes (q, c): the child point; ok[i] is false -- and the outputs 0 -- for a hardened index and for a q that is not on the curve.  Public data.
  static WCP bip32_ckd_pub(WCP const& q, WBN const& c, uint32_t index, WBN& c_child, hip::mask& ok) requires std::is_same_v<Curve, curve_secp256k1> {
    return bip32_ckd_pub_impl(q, c, nullptr, index, c_child, ok);
  }
  static WCP bip32_ckd_pub(WCP const& q, WBN const& c, hip::indices const& index, WBN& c_child, hip::mask& ok) requires std::is_same_v<Curve, curve_secp256k1> {
    same_length(c.size(), index.size(), "bip32_ckd_pub");
    return bip32_ckd_pub_impl(q, c, index.data(), 0, c_child, ok);
  }
  // the node at the end of `path` below the SECRET nodes (k, c): one bip32_ckd_priv per level; ok is the AND of the levels' masks
  static WBN bip32_derive_priv(WBN const& k, WBN const& c, std::vector<uint32_t> const& path, WBN& c_out, hip::mask& ok) requires std::is_same_v<Curve, curve_secp256k1> {
    WBN key = k; c_out = c; ok = hip::mask::filled(k.size(), true);
    for (uint32_t index : path) {
      WBN cc; hip::mask level;
      key = bip32_ckd_priv(key, c_out, index, cc, level);
      c_out = cc;
      ok = ok && level;
    }
    return key;
  }
  // ---- several GPUs: k[i] * P[i] for HOST arrays, sharded over a device group.  P affine classical (x, y);
  // the result is what scalar_mult(x, from_affine(P)) returns lane by lane -- Jacobian, Montgomery form -- or, with
  // affine_out, what .to_affine() of it returns.  Member m computes the slice device_group::shard_range(n, m, size());
  // one gather brings the shards to the first device and the result to the host.
  struct host_points { std::vector<BN> x, y, z; };            // z is empty for affine output
  static host_points scalar_mult(hip::device_group& g, std::vector<BN> const& k, std::vector<BN> const& px, std::vector<BN> const& py, bool affine_out = false) {
    if (k.size() != px.size() || k.size() != py.size()) throw hip::error("ecsimd: scalar_mult over host arrays of different length");
    static_assert(sizeof(BN) == 32, "a 256-bit element is 4 x u64, contiguous");
    const size_t n = k.size();
    host_points r; r.x.resize(n); r.y.resize(n); if (!affine_out) r.z.resize(n);
    auto w = [](std::vector<BN> const& v) { return reinterpret_cast<const uint64_t*>(v.data()); };
    auto m = [](std::vector<BN>& v) { return v.empty() ? nullptr : reinterpret_cast<uint64_t*>(v.data()); };
    g.check(ecsimd_hip_group_scalar_mult_host(g.handle(), curve_id(), w(k), w(px), w(py), m(r.x), m(r.y), m(r.z), n,
                                              ECSIMD_HIP_BASE_CLASSICAL | (affine_out ? ECSIMD_HIP_OUT_AFFINE : ECSIMD_HIP_OUT_JACOBIAN)), "ecsimd_hip_group_scalar_mult_host");
    return r;
  }
 private:
  static WBN bip32_ckd_priv_impl(WBN const& k, WBN const& c, const uint32_t* index, uint32_t index_all, WBN& c_child, hip::mask& ok, int flags) {
    same_length(k.size(), c.size(), "bip32_ckd_priv");
    auto out = WBN::uninitialized(k.size()); c_child = WBN::uninitialized(k.size()); ok = hip::mask(k.size());
    hip::check(ecsimd_hip_bip32_ckd_priv(hip::context(), k.data(), c.data(), index, index_all, out.data(), c_child.data(), ok.data(), k.size(), flags), "ecsimd_hip_bip32_ckd_priv");
    return out;
  }
  static WCP bip32_ckd_pub_impl(WCP const& q, WBN const& c, const uint32_t* index, uint32_t index_all, WBN& c_child, hip::mask& ok) {
    same_length(q.x().size(), c.size(), "bip32_ckd_pub");
    auto cx = WBN::uninitialized(c.size()); auto cy = WBN::uninitialized(c.size()); c_child = WBN::uninitialized(c.size()); ok = hip::mask(c.size());
    hip::check(ecsimd_hip_bip32_ckd_pub(hip::context(), q.x().data(), q.y().data(), c.data(), index, index_all, cx.data(), cy.data(), c_child.data(), ok.data(), c.size()),
               "ecsimd_hip_bip32_ckd_pub");
    return WCP{cx, cy};
  }
  // The C ABI takes one length for all operands (in the reference it is a property of the type): a shorter batch would be
  // read or written out of bounds on the device.
  static void same_length(size_t a, size_t b, const char* what) {
    if (a != b) throw hip::error(std::string("ecsimd: ") + what + " over batches of different length");
  }
  static WJCP fresh_xy(size_t n) {                  // z is attached by the caller (a shared co-Z array)
    WJCP r; r.x() = gfp{WMBN{WBN::uninitialized(n)}}; r.y() = gfp{WMBN{WBN::uninitialized(n)}}; return r;
  }
  static WJCP fresh(size_t n) {
    WJCP r; r.x() = gfp{WMBN{WBN::uninitialized(n)}}; r.y() = gfp{WMBN{WBN::uninitialized(n)}}; r.z() = gfp{WMBN{WBN::uninitialized(n)}}; return r;
  }
  static uint64_t* px(WJCP const& p) { return p.x().wbn().data(); }
  static uint64_t* py(WJCP const& p) { return p.y().wbn().data(); }
  static uint64_t* pz(WJCP const& p) { return p.z().wbn().data(); }
};
}  // namespace ecsimd
#endif
