// ecsimd/sha512.h -- batched SHA-512 and HMAC-SHA-512 on the device (ecsimd_hip_sha512, ecsimd_hip_hmac_sha512; not in the reference) over n equal-length
// messages, as a device array of 64-byte digests, and the device array of 32-bit child indices that the BIP-32 members of
// curve_group<curve_secp256k1> take.  Public data only -- except hip::pbkdf2_hmac_sha512 and hip::bip39_seed (ecsimd_hip_pbkdf2_hmac_sha512,
// ecsimd_hip_bip39_seed), whose passwords, salts and derived keys are SECRET and whose lengths are public.
#ifndef ECSIMD_SHA512_H
#define ECSIMD_SHA512_H
#include <ecsimd/sha256.h>
#include <array>
#include <vector>

namespace ecsimd {
namespace hip {
// n digests of 64 bytes in device memory, packed
class digests64 {
 public:
  using digest = std::array<uint8_t, 64>;
  digests64() = default;
  explicit digests64(size_t n) : mem_(8 * n), n_(n) {}
  uint8_t* data() const { return reinterpret_cast<uint8_t*>(mem_.data()); }
  size_t size() const { return n_; }
  std::vector<digest> host() const {
    std::vector<digest> h(n_);
    if (n_) check(ecsimd_hip_memcpy_d2h(context(), h.data(), mem_.data(), 64 * n_), "d2h");
    return h;
  }
  digest get(size_t i) const { return host().at(i); }
 private:
  buffer mem_;
  size_t n_ = 0;
};

inline digests64 sha512(messages const& m) {
  digests64 out(m.size());
  check(ecsimd_hip_sha512(context(), m.data(), m.msg_bytes(), m.stride_bytes(), out.data(), m.size()), "ecsimd_hip_sha512");
  return out;
}
// one key per message (keys.size() == m.size()), or ONE key for all of them (keys.size() == 1)
inline digests64 hmac_sha512(messages const& keys, messages const& m) {
  if (keys.size() != m.size() && keys.size() != 1) throw error("ecsimd: hmac_sha512 takes one key, or one key per message");
  digests64 out(m.size());
  check(ecsimd_hip_hmac_sha512(context(), keys.data(), keys.msg_bytes(), keys.size() == 1 ? 0 : keys.stride_bytes(), m.data(), m.msg_bytes(), m.stride_bytes(), out.data(), m.size()),
        "ecsimd_hip_hmac_sha512");
  return out;
}

// n derived keys of key_bytes bytes each in device memory, packed
class derived_keys {
 public:
  derived_keys() = default;
  derived_keys(size_t n, size_t key_bytes) : mem_((n * key_bytes + 7) / 8), n_(n), key_bytes_(key_bytes) {}
  uint8_t* data() const { return reinterpret_cast<uint8_t*>(mem_.data()); }
  size_t size() const { return n_; }
  size_t key_bytes() const { return key_bytes_; }
  std::vector<std::vector<uint8_t>> host() const {
    std::vector<uint8_t> flat(n_ * key_bytes_);
    if (!flat.empty()) check(ecsimd_hip_memcpy_d2h(context(), flat.data(), mem_.data(), flat.size()), "d2h");
    std::vector<std::vector<uint8_t>> h(n_);
    for (size_t i = 0; i < n_; ++i) h[i].assign(flat.begin() + i * key_bytes_, flat.begin() + (i + 1) * key_bytes_);
    return h;
  }
  std::vector<uint8_t> get(size_t i) const { return host().at(i); }
 private:
  buffer mem_;
  size_t n_ = 0, key_bytes_ = 0;
};
// PBKDF2-HMAC-SHA-512 (RFC 8018) of n equal-length SECRET passwords: one salt per password (salts.size() == passwords.size()) or ONE salt for all (salts.size() == 1)
inline derived_keys pbkdf2_hmac_sha512(messages const& passwords, messages const& salts, uint32_t iterations, size_t dk_bytes) {
  if (salts.size() != passwords.size() && salts.size() != 1) throw error("ecsimd: pbkdf2_hmac_sha512 takes one salt, or one salt per password");
  derived_keys out(passwords.size(), dk_bytes);
  check(ecsimd_hip_pbkdf2_hmac_sha512(context(), passwords.data(), passwords.msg_bytes(), passwords.stride_bytes(), nullptr, salts.data(), salts.msg_bytes(),
                                      salts.size() == 1 ? 0 : salts.stride_bytes(), nullptr, iterations, out.data(), dk_bytes, dk_bytes, passwords.size()), "ecsimd_hip_pbkdf2_hmac_sha512");
  return out;
}
// The BIP-39 seeds (64 bytes) of n equal-length SECRET sentences, taken as bytes (NFKD, the word list and the checksum are the caller's): one passphrase per
// sentence, or ONE for all (passphrases.size() == 1; an empty one: messages(nullptr, 1, 0, 0))
inline derived_keys bip39_seed(messages const& mnemonics, messages const& passphrases) {
  if (passphrases.size() != mnemonics.size() && passphrases.size() != 1) throw error("ecsimd: bip39_seed takes one passphrase, or one passphrase per sentence");
  derived_keys out(mnemonics.size(), 64);
  check(ecsimd_hip_bip39_seed(context(), mnemonics.data(), mnemonics.msg_bytes(), mnemonics.stride_bytes(), nullptr, passphrases.msg_bytes() ? passphrases.data() : nullptr,
                              passphrases.msg_bytes(), passphrases.size() == 1 ? 0 : passphrases.stride_bytes(), nullptr, out.data(), mnemonics.size()), "ecsimd_hip_bip39_seed");
  return out;
}

// n BIP-32 child indices in device memory (i >= 2^31: hardened), copied from the host
using indices = lengths;
}  // namespace hip
}  // namespace ecsimd
#endif
