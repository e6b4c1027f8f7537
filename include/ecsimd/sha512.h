// ecsimd/sha512.h -- batched SHA-512 and HMAC-SHA-512 on the device (ecsimd_hip_sha512, ecsimd_hip_hmac_sha512; not in the reference) over n equal-length
// messages, as a device array of 64-byte digests, and the device array of 32-bit child indices that the BIP-32 members of
// curve_group<curve_secp256k1> take.  Public data only.
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

// n BIP-32 child indices in device memory (i >= 2^31: hardened), copied from the host
class indices {
 public:
  indices() = default;
  explicit indices(std::vector<uint32_t> const& host) : mem_((host.size() + 1) / 2), n_(host.size()) {
    if (n_) check(ecsimd_hip_memcpy_h2d(context(), mem_.data(), host.data(), 4 * n_), "h2d");
  }
  const uint32_t* data() const { return reinterpret_cast<const uint32_t*>(mem_.data()); }
  size_t size() const { return n_; }
 private:
  buffer mem_;
  size_t n_ = 0;
};
}  // namespace hip
}  // namespace ecsimd
#endif
