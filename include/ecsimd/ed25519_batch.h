// ecsimd/ed25519_batch.h -- Ed25519 batch verification on the device over ecsimd_ed25519_batch.h (not in the reference): hip::ed25519_verify_batch (ONE verdict
// for a batch), hip::ed25519_verify_cofactored (the per-lane rule that names the culprits of a refused batch), hip::ed25519_batch_randomizers,
// hip::ed25519_batch_plan, and the bucket sum on the twisted Edwards curve both stand on: hip::ed25519_msm / hip::ed25519_msm_plan.  Operands are those of
// ecsimd/ed25519.h: hip::byte_records of 32 (keys, scalars, encodings) and 64 bytes (signatures), hip::messages with optional hip::lengths.  The rule is strict
// encodings with the COFACTORED equation (not ZIP-215): ecsimd_ed25519_batch.h states it.  PUBLIC data only.
#ifndef ECSIMD_ED25519_BATCH_CPP_H
#define ECSIMD_ED25519_BATCH_CPP_H
#include <ecsimd/ed25519.h>
#include <ecsimd_ed25519_batch.h>
#include <cstring>

namespace ecsimd {
namespace hip {
// what ed25519_msm(n terms, bits) will do: ecsimd_msm_plan's bucket schedule with this sum's workspace.  Host only: no context, no GPU.
inline ecsimd_msm_plan_t ed25519_msm_plan(size_t n, int bits = 256, int alg = ECSIMD_MSM_ALG_AUTO) {
  ecsimd_msm_plan_t p;
  if (ecsimd_ed25519_msm_plan(n, bits, alg, &p) != ECSIMD_HIP_OK) throw error("ecsimd_ed25519_msm_plan: bits must be 1 .. 256, n at most 2^24, alg AUTO or BUCKETS (the bucket route only)");
  return p;
}
// the sum of (k[i] mod 2^bits) P[i]: its 32-byte encoding, whether it is another point than the identity, and how many encodings did not decode (and contributed nothing)
struct ed25519_msm_result { std::vector<uint8_t> encoding; bool finite; uint32_t invalid; };
inline ed25519_msm_result ed25519_msm(byte_records const& k, byte_records const& pts, int bits = 256, int alg = ECSIMD_MSM_ALG_AUTO) {
  if (k.size() != pts.size() || (k.size() && (k.width() != 32 || pts.width() != 32))) throw error("ecsimd: ed25519_msm: one 32-byte scalar per 32-byte encoding");
  byte_records out(1, 32), invalid(1, 4);
  mask finite(1);
  check(ecsimd_ed25519_msm(context(), k.data(), pts.data(), out.data(), finite.data(), reinterpret_cast<uint32_t*>(invalid.data()), k.size(), bits, alg), "ecsimd_ed25519_msm");
  ed25519_msm_result r{out.get(0), finite.get(0) != 0, 0};
  const std::vector<uint8_t> count = invalid.get(0);
  std::memcpy(&r.invalid, count.data(), 4);
  return r;
}
// one byte per lane: 1 where s < L, A and R decode strictly and [8]([s]B - [h]A - R) is the identity
inline mask ed25519_verify_cofactored(byte_records const& pk, messages const& m, byte_records const& sig, const lengths* lens = nullptr, bool reject_small_order = false) {
  detail::ed25519_sizes(pk.size(), m, lens, pk, 32, "ed25519_verify_cofactored");
  detail::ed25519_sizes(pk.size(), m, lens, sig, 64, "ed25519_verify_cofactored");
  mask ok(pk.size());
  check(ecsimd_ed25519_verify_cofactored(context(), pk.data(), m.data(), m.msg_bytes(), m.stride_bytes(), lens ? lens->data() : nullptr, sig.data(), ok.data(), pk.size(),
                                         reject_small_order ? ECSIMD_ED25519_REJECT_SMALL_ORDER : 0), "ecsimd_ed25519_verify_cofactored");
  return ok;
}
// what ed25519_verify_batch(n signatures, messages of at most msg_bytes bytes, flags) will do: the route, the launches, the workspace.  Host only.
inline ecsimd_ed25519_batch_plan_t ed25519_batch_plan(size_t n, size_t msg_bytes, int flags = ECSIMD_ED25519_BATCH_AUTO) {
  ecsimd_ed25519_batch_plan_t p;
  if (ecsimd_ed25519_batch_plan(n, msg_bytes, flags, &p) != ECSIMD_HIP_OK)
    throw error("ecsimd_ed25519_batch_plan: n at most 2^24 - 1, msg_bytes at most 2^40, flags AUTO, MSM or LANES, or-able with ECSIMD_ED25519_REJECT_SMALL_ORDER");
  return p;
}
// a mask of ONE lane: true iff every lane passes ed25519_verify_cofactored's rule (up to 2^-127 on the MSM route).  Stream-ordered; nothing is read back.
inline mask ed25519_verify_batch(byte_records const& pk, messages const& m, byte_records const& sig, const lengths* lens = nullptr, int flags = ECSIMD_ED25519_BATCH_AUTO) {
  detail::ed25519_sizes(pk.size(), m, lens, pk, 32, "ed25519_verify_batch");
  detail::ed25519_sizes(pk.size(), m, lens, sig, 64, "ed25519_verify_batch");
  mask ok(1);
  check(ecsimd_ed25519_verify_batch(context(), pk.data(), m.data(), m.msg_bytes(), m.stride_bytes(), lens ? lens->data() : nullptr, sig.data(), ok.data(), pk.size(), flags),
        "ecsimd_ed25519_verify_batch");
  return ok;
}
// the randomizers z_i the MSM route weighs the lanes with: n records of 32 little-endian bytes (odd, below 2^128)
inline byte_records ed25519_batch_randomizers(byte_records const& pk, messages const& m, byte_records const& sig, const lengths* lens = nullptr) {
  detail::ed25519_sizes(pk.size(), m, lens, pk, 32, "ed25519_batch_randomizers");
  detail::ed25519_sizes(pk.size(), m, lens, sig, 64, "ed25519_batch_randomizers");
  byte_records z(pk.size(), 32);
  check(ecsimd_ed25519_batch_randomizers(context(), pk.data(), m.data(), m.msg_bytes(), m.stride_bytes(), lens ? lens->data() : nullptr, sig.data(), z.data(), pk.size()),
        "ecsimd_ed25519_batch_randomizers");
  return z;
}
}  // namespace hip
}  // namespace ecsimd
#endif
