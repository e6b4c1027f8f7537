// ecsimd/p384.h -- batched NIST P-384 on the device: hip::p384_sha384 / p384_pubkey / p384_ecdh / p384_ecdsa_verify / p384_ecdsa_sign over ecsimd_p384.h
// (not in the reference).  Private keys, digests and shared secrets are hip::byte_records of 48 big-endian bytes, public keys (X || Y) and signatures
// (r || s) of 96.  The private keys are SECRET (what that means on the device: ecsimd_p384.h).  Every call that can refuse a lane returns its `ok` mask.
#ifndef ECSIMD_P384_CPP_H
#define ECSIMD_P384_CPP_H
#include <ecsimd/ed25519.h>
#include <ecsimd_p384.h>
#include <utility>

namespace ecsimd {
namespace hip {
namespace detail {
inline void p384_sizes(byte_records const& a, size_t n, size_t width, const char* what) {
  if (a.width() != width || a.size() != n) throw error(std::string("ecsimd: ") + what + ": records of " + std::to_string(width) + " bytes, one per lane");
}
}  // namespace detail

// the SHA-384 digests (48 bytes) of the messages; lens: one length per lane (hip::ragged)
inline byte_records p384_sha384(messages const& m, const lengths* lens = nullptr) {
  if (lens && lens->size() != m.size()) throw error("ecsimd: p384_sha384: operands disagree on the batch");
  byte_records out(m.size(), 48);
  check(ecsimd_p384_sha384(context(), m.data(), m.msg_bytes(), m.stride_bytes(), lens ? lens->data() : nullptr, out.data(), m.size()), "ecsimd_p384_sha384");
  return out;
}
// (public keys X || Y, ok) of the SECRET private keys; ok is 0, and the key zero, where d is not in [1, n - 1]
inline std::pair<byte_records, mask> p384_pubkey(byte_records const& d) {
  detail::p384_sizes(d, d.size(), 48, "p384_pubkey");
  byte_records pub(d.size(), 96);
  mask ok(d.size());
  check(ecsimd_p384_pubkey(context(), d.data(), pub.data(), ok.data(), d.size()), "ecsimd_p384_pubkey");
  return {pub, ok};
}
// (z = x(d peer), ok); ok is 0, and z zero, where d is not in [1, n - 1] or the peer does not decode
inline std::pair<byte_records, mask> p384_ecdh(byte_records const& d, byte_records const& peer) {
  detail::p384_sizes(d, d.size(), 48, "p384_ecdh");
  detail::p384_sizes(peer, d.size(), 96, "p384_ecdh");
  byte_records z(d.size(), 48);
  mask ok(d.size());
  check(ecsimd_p384_ecdh(context(), d.data(), peer.data(), z.data(), ok.data(), d.size()), "ecsimd_p384_ecdh");
  return {z, ok};
}
// one byte per lane: 1 where the signature r || s of the 48-byte digest is accepted under the public key
inline mask p384_ecdsa_verify(byte_records const& pub, byte_records const& digest, byte_records const& sig) {
  detail::p384_sizes(pub, pub.size(), 96, "p384_ecdsa_verify");
  detail::p384_sizes(digest, pub.size(), 48, "p384_ecdsa_verify");
  detail::p384_sizes(sig, pub.size(), 96, "p384_ecdsa_verify");
  mask ok(pub.size());
  check(ecsimd_p384_ecdsa_verify(context(), pub.data(), digest.data(), sig.data(), ok.data(), pub.size()), "ecsimd_p384_ecdsa_verify");
  return ok;
}
// (signatures r || s, ok): deterministic ECDSA (RFC 6979, HMAC-SHA-384, one candidate) of the 48-byte digests under the SECRET private keys
inline std::pair<byte_records, mask> p384_ecdsa_sign(byte_records const& d, byte_records const& digest) {
  detail::p384_sizes(d, d.size(), 48, "p384_ecdsa_sign");
  detail::p384_sizes(digest, d.size(), 48, "p384_ecdsa_sign");
  byte_records sig(d.size(), 96);
  mask ok(d.size());
  check(ecsimd_p384_ecdsa_sign(context(), d.data(), digest.data(), sig.data(), ok.data(), d.size(), 0), "ecsimd_p384_ecdsa_sign");
  return {sig, ok};
}
}  // namespace hip
}  // namespace ecsimd
#endif
