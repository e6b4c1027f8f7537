// ecsimd/sha256.h -- batched SHA-256 on the device (ecsimd_hip_sha256, ecsimd_hip_sha256_lens; not in the reference): the digests of n messages -- of one length, or
// with a length each -- as the 256-bit
// integers the ECDSA calls of curve_group<Curve> take as `e`, made where the signatures are made and checked.
#ifndef ECSIMD_SHA256_H
#define ECSIMD_SHA256_H
#include <ecsimd/bignum.h>
#include <algorithm>
#include <string>
#include <utility>
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

// n x u32 in device memory, copied from the host: one length per message (the lens of the *_lens calls), BIP-32's child indices
class lengths {
 public:
  lengths() = default;
  explicit lengths(std::vector<uint32_t> const& host) : mem_((host.size() + 1) / 2), n_(host.size()) {
    if (n_) check(ecsimd_hip_memcpy_h2d(context(), mem_.data(), host.data(), 4 * n_), "h2d");
  }
  const uint32_t* data() const { return reinterpret_cast<const uint32_t*>(mem_.data()); }
  size_t size() const { return n_; }
 private:
  buffer mem_;
  size_t n_ = 0;
};
// Messages of any lengths as rows of one stride (the longest length, rounded up to a multiple of 4: word loads), with their lengths
inline std::pair<messages, lengths> ragged(std::vector<std::string> const& m) {
  size_t stride = 4;
  for (auto const& s : m) stride = std::max(stride, (s.size() + 3) / 4 * 4);
  std::vector<uint8_t> flat(m.size() * stride + 1, 0);
  std::vector<uint32_t> lens;
  for (size_t i = 0; i < m.size(); ++i) { std::copy(m[i].begin(), m[i].end(), flat.begin() + i * stride); lens.push_back((uint32_t)m[i].size()); }
  return {messages(flat.data(), m.size(), stride, stride), lengths(lens)};
}
inline void same_rows(messages const& m, lengths const& lens) { if (m.size() != lens.size()) throw error("ecsimd: messages and lengths of different number"); }

// e[i] = SHA-256(message i) as an integer: the digest read as a big-endian number
inline wide_bignum<bignum_256> sha256(messages const& m) {
  auto e = wide_bignum<bignum_256>::uninitialized(m.size());
  check(ecsimd_hip_sha256(context(), m.data(), m.msg_bytes(), m.stride_bytes(), e.data(), m.size()), "ecsimd_hip_sha256");
  return e;
}
// ... of the first lens[i] bytes of message i (ecsimd_hip_sha256_lens)
inline wide_bignum<bignum_256> sha256(messages const& m, lengths const& lens) {
  same_rows(m, lens);
  auto e = wide_bignum<bignum_256>::uninitialized(m.size());
  check(ecsimd_hip_sha256_lens(context(), m.data(), m.msg_bytes(), m.stride_bytes(), lens.data(), e.data(), m.size()), "ecsimd_hip_sha256_lens");
  return e;
}
}  // namespace hip
}  // namespace ecsimd
#endif
