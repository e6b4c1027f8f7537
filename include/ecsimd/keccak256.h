// ecsimd/keccak256.h -- batched Keccak-256 on the device (ecsimd_hip_keccak256; not in the reference): Ethereum's hash -- the original Keccak padding, not
// NIST's SHA-3 -- of n equal-length messages as the 256-bit integers the ECDSA calls of curve_group<Curve> take as `e`, and the device array of 20-byte
// addresses that curve_group<curve_secp256k1>::eth_address / eth_recover return.  Public data only.
#ifndef ECSIMD_KECCAK256_H
#define ECSIMD_KECCAK256_H
#include <ecsimd/sha256.h>
#include <array>
#include <vector>

namespace ecsimd {
namespace hip {
// e[i] = Keccak-256(message i) as an integer: the digest read as a big-endian number
inline wide_bignum<bignum_256> keccak256(messages const& m) {
  auto e = wide_bignum<bignum_256>::uninitialized(m.size());
  check(ecsimd_hip_keccak256(context(), m.data(), m.msg_bytes(), m.stride_bytes(), nullptr, e.data(), m.size()), "ecsimd_hip_keccak256");
  return e;
}

// n Ethereum addresses in device memory, 20 bytes each, packed
class addresses {
 public:
  using address = std::array<uint8_t, 20>;
  addresses() = default;
  explicit addresses(size_t n) : mem_((20 * n + 7) / 8), n_(n) {}
  uint8_t* data() const { return reinterpret_cast<uint8_t*>(mem_.data()); }
  size_t size() const { return n_; }
  std::vector<address> host() const {
    std::vector<address> h(n_);
    if (n_) check(ecsimd_hip_memcpy_d2h(context(), h.data(), mem_.data(), 20 * n_), "d2h");
    return h;
  }
  address get(size_t i) const { return host().at(i); }
 private:
  buffer mem_;
  size_t n_ = 0;
};
}  // namespace hip
}  // namespace ecsimd
#endif
