// ecsimd/x25519.h -- batched X25519 (RFC 7748) on the device: hip::x25519 / x25519_base / x25519_from_ed25519_pk / x25519_from_ed25519_seed over
// ecsimd_x25519.h (not in the reference).  Scalars, u-coordinates, shared secrets, seeds and Ed25519 keys are hip::byte_records of 32 bytes.  The scalars and
// seeds are SECRET (what that means on the device: ecsimd_x25519.h).  A shared secret of 32 zero bytes means the peer's u had small order: pass `ok` and read it.
#ifndef ECSIMD_X25519_CPP_H
#define ECSIMD_X25519_CPP_H
#include <ecsimd/ed25519.h>
#include <ecsimd_x25519.h>
#include <utility>

namespace ecsimd {
namespace hip {
namespace detail {
inline void x25519_sizes(byte_records const& a, size_t n, const char* what) {
  if (a.width() != 32 || a.size() != n) throw error(std::string("ecsimd: ") + what + ": records of 32 bytes, one per lane");
}
}  // namespace detail

// the shared secrets X25519(scalar, u); ok (optional): one byte per lane, 0 where the secret is all zero (RFC 7748 section 6.1's check)
inline byte_records x25519(byte_records const& scalars, byte_records const& us, mask* ok = nullptr) {
  detail::x25519_sizes(scalars, scalars.size(), "x25519");
  detail::x25519_sizes(us, scalars.size(), "x25519");
  byte_records out(scalars.size(), 32);
  if (ok) *ok = mask(scalars.size());
  check(ecsimd_x25519(context(), scalars.data(), us.data(), out.data(), ok ? ok->data() : nullptr, scalars.size()), "ecsimd_x25519");
  return out;
}
// the public keys X25519(scalar, 9)
inline byte_records x25519_base(byte_records const& scalars) {
  detail::x25519_sizes(scalars, scalars.size(), "x25519_base");
  byte_records out(scalars.size(), 32);
  check(ecsimd_x25519_base(context(), scalars.data(), out.data(), scalars.size()), "ecsimd_x25519_base");
  return out;
}
// (u, ok) of Ed25519 public keys: ok is 0, and u zero, where a key does not decode strictly or has small order.  No prime-subgroup check.
inline std::pair<byte_records, mask> x25519_from_ed25519_pk(byte_records const& pk) {
  detail::x25519_sizes(pk, pk.size(), "x25519_from_ed25519_pk");
  byte_records u(pk.size(), 32);
  mask ok(pk.size());
  check(ecsimd_x25519_from_ed25519_pk(context(), pk.data(), u.data(), ok.data(), pk.size()), "ecsimd_x25519_from_ed25519_pk");
  return {u, ok};
}
// the X25519 private keys of Ed25519 seeds: the clamped low half of SHA-512(seed)
inline byte_records x25519_from_ed25519_seed(byte_records const& seeds) {
  detail::x25519_sizes(seeds, seeds.size(), "x25519_from_ed25519_seed");
  byte_records out(seeds.size(), 32);
  check(ecsimd_x25519_from_ed25519_seed(context(), seeds.data(), out.data(), seeds.size()), "ecsimd_x25519_from_ed25519_seed");
  return out;
}
}  // namespace hip
}  // namespace ecsimd
#endif
