// ecsimd/sha256.h -- batched SHA-256 on the device (ecsimd_hip_sha256; not in the reference): the digests of n equal-length messages as the 256-bit
// integers the ECDSA calls of curve_group<Curve> take as `e`, made where the signatures are made and checked.
#ifndef ECSIMD_SHA256_H
#define ECSIMD_SHA256_H
#include <ecsimd/bignum.h>
#include <string>
#include <vector>

namespace ecsimd {
namespace hip {
// n messages of msg_bytes bytes each in device memory, message i at data() + i * stride_bytes() (a record array whose records begin with the message:
// stride_bytes > msg_bytes).  Copied from host memory laid out the same way.
class messages {
 public:
  messages(const uint8_t* host, size_t n, size_t msg_bytes, size_t stride_bytes) : n_(n), msg_bytes_(msg_bytes), stride_(stride_bytes) {
    if (stride_bytes < msg_bytes) throw error("ecsimd: messages with a stride below their length");
    const size_t bytes = n ? (n - 1) * stride_bytes + msg_bytes : 0;
    mem_ = buffer((bytes + 7) / 8);
    if (bytes) check(ecsimd_hip_memcpy_h2d(context(), mem_.data(), host, bytes), "h2d");
  }
  // equal-length strings, packed
  explicit messages(std::vector<std::string> const& m) : messages(pack(m).data(), m.size(), m.empty() ? 0 : m[0].size(), m.empty() ? 0 : m[0].size()) {}
  const uint8_t* data() const { return reinterpret_cast<const uint8_t*>(mem_.data()); }
  size_t size() const { return n_; }
  size_t msg_bytes() const { return msg_bytes_; }
  size_t stride_bytes() const { return stride_; }
 private:
  static std::vector<uint8_t> pack(std::vector<std::string> const& m) {
    std::vector<uint8_t> flat;
    for (auto const& s : m) { if (s.size() != m[0].size()) throw error("ecsimd: sha256 takes messages of ONE length"); flat.insert(flat.end(), s.begin(), s.end()); }
    if (flat.empty()) flat.push_back(0);
    return flat;
  }
  buffer mem_;
  size_t n_ = 0, msg_bytes_ = 0, stride_ = 0;
};

// e[i] = SHA-256(message i) as an integer: the digest read as a big-endian number
inline wide_bignum<bignum_256> sha256(messages const& m) {
  auto e = wide_bignum<bignum_256>::uninitialized(m.size());
  check(ecsimd_hip_sha256(context(), m.data(), m.msg_bytes(), m.stride_bytes(), e.data(), m.size()), "ecsimd_hip_sha256");
  return e;
}
}  // namespace hip
}  // namespace ecsimd
#endif
