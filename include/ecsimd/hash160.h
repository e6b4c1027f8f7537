// ecsimd/hash160.h -- Bitcoin's hashes on the device (ecsimd_hip_ripemd160, ecsimd_hip_hash160, ecsimd_hip_sha256d; not in the reference) over n equal-length
// messages: RIPEMD-160 and HASH160 = RIPEMD-160(SHA-256(m)) as a device array of 20-byte digests, the double SHA-256 as the 256-bit integers hip::sha256
// returns.  curve_group<curve_secp256k1>::btc_pubkey_hash returns the same array type.  Public data only.
#ifndef ECSIMD_HASH160_H
#define ECSIMD_HASH160_H
#include <ecsimd/keccak256.h>

namespace ecsimd {
namespace hip {
// n digests of 20 bytes in device memory, packed: the array type of the Ethereum addresses
using digests20 = addresses;

inline digests20 ripemd160(messages const& m) {
  digests20 out(m.size());
  check(ecsimd_hip_ripemd160(context(), m.data(), m.msg_bytes(), m.stride_bytes(), out.data(), m.size()), "ecsimd_hip_ripemd160");
  return out;
}
inline digests20 hash160(messages const& m) {
  digests20 out(m.size());
  check(ecsimd_hip_hash160(context(), m.data(), m.msg_bytes(), m.stride_bytes(), out.data(), m.size()), "ecsimd_hip_hash160");
  return out;
}
// e[i] = SHA-256(SHA-256(message i)) as an integer: the digest read as a big-endian number
inline wide_bignum<bignum_256> sha256d(messages const& m) {
  auto e = wide_bignum<bignum_256>::uninitialized(m.size());
  check(ecsimd_hip_sha256d(context(), m.data(), m.msg_bytes(), m.stride_bytes(), e.data(), m.size()), "ecsimd_hip_sha256d");
  return e;
}
// The same three of the first lens[i] bytes of message i (ecsimd_hip_ripemd160_lens, _hash160_lens, _sha256d_lens): transactions, scripts, witness items
inline digests20 ripemd160(messages const& m, lengths const& lens) {
  same_rows(m, lens);
  digests20 out(m.size());
  check(ecsimd_hip_ripemd160_lens(context(), m.data(), m.msg_bytes(), m.stride_bytes(), lens.data(), out.data(), m.size()), "ecsimd_hip_ripemd160_lens");
  return out;
}
inline digests20 hash160(messages const& m, lengths const& lens) {
  same_rows(m, lens);
  digests20 out(m.size());
  check(ecsimd_hip_hash160_lens(context(), m.data(), m.msg_bytes(), m.stride_bytes(), lens.data(), out.data(), m.size()), "ecsimd_hip_hash160_lens");
  return out;
}
inline wide_bignum<bignum_256> sha256d(messages const& m, lengths const& lens) {
  same_rows(m, lens);
  auto e = wide_bignum<bignum_256>::uninitialized(m.size());
  check(ecsimd_hip_sha256d_lens(context(), m.data(), m.msg_bytes(), m.stride_bytes(), lens.data(), e.data(), m.size()), "ecsimd_hip_sha256d_lens");
  return e;
}
}  // namespace hip
}  // namespace ecsimd
#endif
