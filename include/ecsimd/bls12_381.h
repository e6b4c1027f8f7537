// ecsimd/bls12_381.h -- BLS12-381 G1 on the device over ecsimd_bls12_381.h (not in the reference): hip::bls12_381::g1_decompress / g1_compress / g1_check /
// g1_mul per lane, g1_msm and g1_point_sum across lanes, g1_msm_plan on the host.  Points are hip::byte_records of 96 bytes (uncompressed) or 48 (compressed) in
// the ZCash / IETF serialisation; scalars are hip::byte_records of 32 LITTLE-ENDIAN bytes (the limbs of the C ABI as they lie in memory; a byte_records
// allocation is 16-byte aligned).  PUBLIC data only; validation is on-curve only except in g1_check (ecsimd_bls12_381.h).
#ifndef ECSIMD_BLS12_381_CPP_H
#define ECSIMD_BLS12_381_CPP_H
#include <ecsimd/ed25519.h>
#include <ecsimd_bls12_381.h>
#include <cstring>
#include <utility>

namespace ecsimd {
namespace hip {
namespace bls12_381 {
namespace detail {
inline void sizes(byte_records const& a, size_t n, size_t width, const char* what) {
  if (a.size() != n || (n && a.width() != width)) throw error(std::string("ecsimd: bls12_381::") + what + ": records of " + std::to_string(width) + " bytes, one per lane");
}
inline const uint64_t* limbs(byte_records const& k) { return reinterpret_cast<const uint64_t*>(k.data()); }
}  // namespace detail

// (uncompressed points, ok) of the compressed ones; a malformed lane is zeros with ok = 0
inline std::pair<byte_records, mask> g1_decompress(byte_records const& in48) {
  detail::sizes(in48, in48.size(), 48, "g1_decompress");
  byte_records out(in48.size(), 96);
  mask ok(in48.size());
  check(ecsimd_bls12_381_g1_decompress(context(), in48.data(), out.data(), ok.data(), in48.size()), "ecsimd_bls12_381_g1_decompress");
  return {out, ok};
}
// (compressed points, ok) of the uncompressed ones, validated the same way
inline std::pair<byte_records, mask> g1_compress(byte_records const& in96) {
  detail::sizes(in96, in96.size(), 96, "g1_compress");
  byte_records out(in96.size(), 48);
  mask ok(in96.size());
  check(ecsimd_bls12_381_g1_compress(context(), in96.data(), out.data(), ok.data(), in96.size()), "ecsimd_bls12_381_g1_compress");
  return {out, ok};
}
// (on the curve, in the subgroup) per lane; the second is [r] P = infinity
inline std::pair<mask, mask> g1_check(byte_records const& in96) {
  detail::sizes(in96, in96.size(), 96, "g1_check");
  mask on(in96.size()), sub(in96.size());
  check(ecsimd_bls12_381_g1_check(context(), in96.data(), on.data(), sub.data(), in96.size()), "ecsimd_bls12_381_g1_check");
  return {on, sub};
}
// (k[i] P[i], ok) for the 256-bit integers k
inline std::pair<byte_records, mask> g1_mul(byte_records const& k, byte_records const& in96) {
  detail::sizes(k, in96.size(), 32, "g1_mul");
  detail::sizes(in96, in96.size(), 96, "g1_mul");
  byte_records out(in96.size(), 96);
  mask ok(in96.size());
  check(ecsimd_bls12_381_g1_mul(context(), detail::limbs(k), in96.data(), out.data(), ok.data(), in96.size()), "ecsimd_bls12_381_g1_mul");
  return {out, ok};
}
// what g1_msm(n terms, bits, alg) will do.  Host only: no context, no GPU.
inline ecsimd_msm_plan_t g1_msm_plan(size_t n, int bits = 255, int alg = ECSIMD_MSM_ALG_AUTO) {
  ecsimd_msm_plan_t p;
  if (ecsimd_bls12_381_g1_msm_plan(n, bits, alg, &p) != ECSIMD_HIP_OK) throw error("ecsimd_bls12_381_g1_msm_plan: bits must be 1 .. 256, n at most 2^24, alg AUTO, BUCKETS or LANES");
  return p;
}
// a sum across lanes: its 96-byte encoding, whether it is another point than infinity, and how many points were malformed (and contributed nothing)
struct g1_sum_result { std::vector<uint8_t> encoding; bool finite; uint32_t invalid; };
namespace detail {
template <class Call> g1_sum_result sum(Call call, const char* what) {
  byte_records out(1, 96), invalid(1, 4);
  mask finite(1);
  check(call(out.data(), finite.data(), reinterpret_cast<uint32_t*>(invalid.data())), what);
  g1_sum_result r{out.get(0), finite.get(0) != 0, 0};
  const std::vector<uint8_t> count = invalid.get(0);
  std::memcpy(&r.invalid, count.data(), 4);
  return r;
}
}  // namespace detail
// the sum of (k[i] mod 2^bits) P[i]
inline g1_sum_result g1_msm(byte_records const& k, byte_records const& pts96, int bits = 255, int alg = ECSIMD_MSM_ALG_AUTO) {
  detail::sizes(k, pts96.size(), 32, "g1_msm");
  detail::sizes(pts96, pts96.size(), 96, "g1_msm");
  return detail::sum([&](uint8_t* out, uint8_t* finite, uint32_t* invalid) {
    return ecsimd_bls12_381_g1_msm(context(), detail::limbs(k), pts96.data(), out, finite, invalid, pts96.size(), bits, alg); }, "ecsimd_bls12_381_g1_msm");
}
// the sum of the points: records of 96 bytes, or of 48 (compressed; the width decides)
inline g1_sum_result g1_point_sum(byte_records const& pts) {
  if (pts.size() && pts.width() != 96 && pts.width() != 48) throw error("ecsimd: bls12_381::g1_point_sum: records of 96 or 48 bytes");
  const int flags = pts.width() == 48 ? ECSIMD_BLS12_381_COMPRESSED : ECSIMD_BLS12_381_UNCOMPRESSED;
  return detail::sum([&](uint8_t* out, uint8_t* finite, uint32_t* invalid) {
    return ecsimd_bls12_381_g1_point_sum(context(), pts.data(), out, finite, invalid, pts.size(), flags); }, "ecsimd_bls12_381_g1_point_sum");
}
}  // namespace bls12_381
}  // namespace hip
}  // namespace ecsimd
#endif
