// ecsimd/bls12_381_g2.h -- BLS12-381 G2 on the device over ecsimd_bls12_381_g2.h (not in the reference): hip::bls12_381::g2_decompress / g2_compress / g2_check /
// g2_mul per lane, g2_msm and g2_point_sum across lanes, g2_msm_plan on the host.  Points are hip::byte_records of 192 bytes (uncompressed) or 96 (compressed) in
// the ZCash / IETF serialisation (c1 before c0); scalars are hip::byte_records of 32 LITTLE-ENDIAN bytes, as g1_mul takes them.  PUBLIC data only; validation is
// on-curve only except in g2_check (ecsimd_bls12_381_g2.h).
#ifndef ECSIMD_BLS12_381_G2_CPP_H
#define ECSIMD_BLS12_381_G2_CPP_H
#include <ecsimd/bls12_381.h>
#include <ecsimd_bls12_381_g2.h>

namespace ecsimd {
namespace hip {
namespace bls12_381 {

// (uncompressed points, ok) of the compressed ones; a malformed lane is zeros with ok = 0
inline std::pair<byte_records, mask> g2_decompress(byte_records const& in96) {
  detail::sizes(in96, in96.size(), 96, "g2_decompress");
  byte_records out(in96.size(), 192);
  mask ok(in96.size());
  check(ecsimd_bls381_g2_decompress(context(), in96.data(), out.data(), ok.data(), in96.size()), "ecsimd_bls381_g2_decompress");
  return {out, ok};
}
// (compressed points, ok) of the uncompressed ones, validated the same way
inline std::pair<byte_records, mask> g2_compress(byte_records const& in192) {
  detail::sizes(in192, in192.size(), 192, "g2_compress");
  byte_records out(in192.size(), 96);
  mask ok(in192.size());
  check(ecsimd_bls381_g2_compress(context(), in192.data(), out.data(), ok.data(), in192.size()), "ecsimd_bls381_g2_compress");
  return {out, ok};
}
// (on the curve, in the subgroup) per lane; the second is [r] Q = infinity
inline std::pair<mask, mask> g2_check(byte_records const& in192) {
  detail::sizes(in192, in192.size(), 192, "g2_check");
  mask on(in192.size()), sub(in192.size());
  check(ecsimd_bls381_g2_check(context(), in192.data(), on.data(), sub.data(), in192.size()), "ecsimd_bls381_g2_check");
  return {on, sub};
}
// (k[i] Q[i], ok) for the 256-bit integers k
inline std::pair<byte_records, mask> g2_mul(byte_records const& k, byte_records const& in192) {
  detail::sizes(k, in192.size(), 32, "g2_mul");
  detail::sizes(in192, in192.size(), 192, "g2_mul");
  byte_records out(in192.size(), 192);
  mask ok(in192.size());
  check(ecsimd_bls381_g2_mul(context(), detail::limbs(k), in192.data(), out.data(), ok.data(), in192.size()), "ecsimd_bls381_g2_mul");
  return {out, ok};
}
// what g2_msm(n terms, bits, alg) will do.  Host only: no context, no GPU.
inline ecsimd_msm_plan_t g2_msm_plan(size_t n, int bits = 255, int alg = ECSIMD_MSM_ALG_AUTO) {
  ecsimd_msm_plan_t p;
  if (ecsimd_bls381_g2_msm_plan(n, bits, alg, &p) != ECSIMD_HIP_OK) throw error("ecsimd_bls381_g2_msm_plan: bits must be 1 .. 256, n at most 2^24, alg AUTO, BUCKETS or LANES");
  return p;
}
// a sum across lanes: its 192-byte encoding, whether it is another point than infinity, and how many points were malformed (and contributed nothing)
struct g2_sum_result { std::vector<uint8_t> encoding; bool finite; uint32_t invalid; };
namespace detail {
template <class Call> g2_sum_result sum2(Call call, const char* what) {
  byte_records out(1, 192), invalid(1, 4);
  mask finite(1);
  check(call(out.data(), finite.data(), reinterpret_cast<uint32_t*>(invalid.data())), what);
  g2_sum_result r{out.get(0), finite.get(0) != 0, 0};
  const std::vector<uint8_t> count = invalid.get(0);
  std::memcpy(&r.invalid, count.data(), 4);
  return r;
}
}  // namespace detail
// the sum of (k[i] mod 2^bits) Q[i]
inline g2_sum_result g2_msm(byte_records const& k, byte_records const& pts192, int bits = 255, int alg = ECSIMD_MSM_ALG_AUTO) {
  detail::sizes(k, pts192.size(), 32, "g2_msm");
  detail::sizes(pts192, pts192.size(), 192, "g2_msm");
  return detail::sum2([&](uint8_t* out, uint8_t* finite, uint32_t* invalid) {
    return ecsimd_bls381_g2_msm(context(), detail::limbs(k), pts192.data(), out, finite, invalid, pts192.size(), bits, alg); }, "ecsimd_bls381_g2_msm");
}
// the sum of the points: records of 192 bytes, or of 96 (compressed; the width decides)
inline g2_sum_result g2_point_sum(byte_records const& pts) {
  if (pts.size() && pts.width() != 192 && pts.width() != 96) throw error("ecsimd: bls12_381::g2_point_sum: records of 192 or 96 bytes");
  const int flags = pts.width() == 96 ? ECSIMD_BLS381_G2_COMPRESSED : ECSIMD_BLS381_G2_UNCOMPRESSED;
  return detail::sum2([&](uint8_t* out, uint8_t* finite, uint32_t* invalid) {
    return ecsimd_bls381_g2_point_sum(context(), pts.data(), out, finite, invalid, pts.size(), flags); }, "ecsimd_bls381_g2_point_sum");
}
}  // namespace bls12_381
}  // namespace hip
}  // namespace ecsimd
#endif
