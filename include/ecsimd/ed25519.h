// ecsimd/ed25519.h -- batched Ed25519 (RFC 8032, pure) on the device: hip::ed25519_pubkey / _sign / _verify over ecsimd_ed25519.h (not in the reference).
// Keys, signatures and seeds are BYTES: device arrays of n records of 32, 64 and 32 bytes (hip::byte_records).  Messages are hip::messages (equal lengths) or
// the pair hip::ragged() makes (one length per lane).  The seeds are SECRET (what that means on the device: ecsimd_ed25519.h); verification is public data
// only and follows that header's rule set: s < L, strict decoding of A, the cofactorless equation, R compared as bytes.
#ifndef ECSIMD_ED25519_CPP_H
#define ECSIMD_ED25519_CPP_H
#include <ecsimd/sha256.h>
#include <ecsimd_ed25519.h>
#include <utility>
#include <vector>

namespace ecsimd {
namespace hip {
// n records of `width` bytes each in device memory, packed
class byte_records {
 public:
  byte_records() = default;
  byte_records(size_t n, size_t width) : mem_((n * width + 7) / 8), n_(n), width_(width) {}
  byte_records(std::vector<std::vector<uint8_t>> const& host, size_t width) : byte_records(host.size(), width) {
    std::vector<uint8_t> flat;
    for (auto const& r : host) { if (r.size() != width) throw error("ecsimd: a byte record of the wrong length"); flat.insert(flat.end(), r.begin(), r.end()); }
    if (!flat.empty()) check(ecsimd_hip_memcpy_h2d(context(), mem_.data(), flat.data(), flat.size()), "h2d");
  }
  uint8_t* data() const { return reinterpret_cast<uint8_t*>(mem_.data()); }
  size_t size() const { return n_; }
  size_t width() const { return width_; }
  std::vector<std::vector<uint8_t>> host() const {
    std::vector<uint8_t> flat(n_ * width_);
    if (!flat.empty()) check(ecsimd_hip_memcpy_d2h(context(), flat.data(), mem_.data(), flat.size()), "d2h");
    std::vector<std::vector<uint8_t>> h(n_);
    for (size_t i = 0; i < n_; ++i) h[i].assign(flat.begin() + i * width_, flat.begin() + (i + 1) * width_);
    return h;
  }
  std::vector<uint8_t> get(size_t i) const { return host().at(i); }
 private:
  buffer mem_;
  size_t n_ = 0, width_ = 0;
};

namespace detail {
inline void ed25519_sizes(size_t n, messages const& m, const lengths* lens, byte_records const& a, size_t width, const char* what) {
  if (a.size() != n || a.width() != width || m.size() != n || (lens && lens->size() != n)) throw error(std::string("ecsimd: ") + what + ": operands disagree on the batch or on a record's length");
}
}  // namespace detail

// the public keys (32 bytes) of n SECRET seeds (32 bytes)
inline byte_records ed25519_pubkey(byte_records const& seeds) {
  if (seeds.width() != 32) throw error("ecsimd: ed25519_pubkey takes seeds of 32 bytes");
  byte_records pk(seeds.size(), 32);
  check(ecsimd_ed25519_pubkey(context(), seeds.data(), pk.data(), seeds.size()), "ecsimd_ed25519_pubkey");
  return pk;
}
// (signatures R || s of 64 bytes, public keys) of the messages under the SECRET seeds; lens: one length per lane (hip::ragged)
inline std::pair<byte_records, byte_records> ed25519_sign(byte_records const& seeds, messages const& m, const lengths* lens = nullptr) {
  detail::ed25519_sizes(seeds.size(), m, lens, seeds, 32, "ed25519_sign");
  byte_records sig(seeds.size(), 64), pk(seeds.size(), 32);
  check(ecsimd_ed25519_sign(context(), seeds.data(), m.data(), m.msg_bytes(), m.stride_bytes(), lens ? lens->data() : nullptr, sig.data(), pk.data(), seeds.size()), "ecsimd_ed25519_sign");
  return {sig, pk};
}
// one byte per lane: 1 where the signature is accepted
inline mask ed25519_verify(byte_records const& pk, messages const& m, byte_records const& sig, const lengths* lens = nullptr, bool reject_small_order = false) {
  detail::ed25519_sizes(pk.size(), m, lens, pk, 32, "ed25519_verify");
  detail::ed25519_sizes(pk.size(), m, lens, sig, 64, "ed25519_verify");
  mask ok(pk.size());
  check(ecsimd_ed25519_verify(context(), pk.data(), m.data(), m.msg_bytes(), m.stride_bytes(), lens ? lens->data() : nullptr, sig.data(), ok.data(), pk.size(),
                              reject_small_order ? ECSIMD_ED25519_REJECT_SMALL_ORDER : 0), "ecsimd_ed25519_verify");
  return ok;
}
}  // namespace hip
}  // namespace ecsimd
#endif
