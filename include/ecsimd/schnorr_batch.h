// ecsimd/schnorr_batch.h -- BIP-340 batch verification on the device over ecsimd_schnorr_batch.h (not in the reference): ONE verdict for a batch of signatures.
// curve_group<curve_secp256k1>::schnorr_verify_batch (ecsimd/curve_group.h) returns that verdict as a bool and so waits for the stream; hip::schnorr_verify_batch
// here leaves the byte on the device, for a caller that goes on enqueueing.  hip::schnorr_batch_plan says what a call will do.  PUBLIC data only.
#ifndef ECSIMD_SCHNORR_BATCH_CPP_H
#define ECSIMD_SCHNORR_BATCH_CPP_H
#include <ecsimd/curve_group.h>
#include <ecsimd_schnorr_batch.h>

namespace ecsimd {
namespace hip {
// what schnorr_verify_batch(n signatures, messages of msg_bytes bytes, route) will do: the route, the launches, the workspace.  Host only: no context, no GPU.
inline ecsimd_schnorr_batch_plan_t schnorr_batch_plan(size_t n, size_t msg_bytes, int route = ECSIMD_SCHNORR_BATCH_AUTO) {
  ecsimd_schnorr_batch_plan_t p;
  if (ecsimd_schnorr_batch_plan(n, msg_bytes, route, &p) != ECSIMD_HIP_OK) throw error("ecsimd_schnorr_batch_plan: n at most 2^24 - 1, msg_bytes at most 2^40, route AUTO, MSM or LANES");
  return p;
}
// a mask of ONE lane: true iff every signature (r, s) of the messages m under the x-only keys px is valid.  Stream-ordered; nothing is read back.
inline mask schnorr_verify_batch(wide_bignum<bignum_256> const& px, messages const& m, wide_bignum<bignum_256> const& r, wide_bignum<bignum_256> const& s,
                                 int route = ECSIMD_SCHNORR_BATCH_AUTO) {
  if (px.size() != m.size() || r.size() != m.size() || s.size() != m.size()) throw error("ecsimd: schnorr_verify_batch: one key, one message, one r and one s per signature");
  mask ok(1);
  check(ecsimd_schnorr_verify_batch(context(), px.data(), m.data(), m.msg_bytes(), m.stride_bytes(), r.data(), s.data(), ok.data(), m.size(), route), "ecsimd_schnorr_verify_batch");
  return ok;
}
}  // namespace hip
}  // namespace ecsimd
#endif
