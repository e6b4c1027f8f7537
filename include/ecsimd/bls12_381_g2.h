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

// every call is ecsimd/bls12_381.h's detail implementation at this group's widths
// (uncompressed points, ok) of the compressed ones; a malformed lane is zeros with ok = 0
inline std::pair<byte_records, mask> g2_decompress(byte_records const& in96) {
  return detail::recode(ecsimd_bls381_g2_decompress, "ecsimd_bls381_g2_decompress", "g2_decompress", in96, 96, 192);
}
// (compressed points, ok) of the uncompressed ones, validated the same way
inline std::pair<byte_records, mask> g2_compress(byte_records const& in192) {
  return detail::recode(ecsimd_bls381_g2_compress, "ecsimd_bls381_g2_compress", "g2_compress", in192, 192, 96);
}
// (on the curve, in the subgroup) per lane; the second is [r] Q = infinity
inline std::pair<mask, mask> g2_check(byte_records const& in192) { return detail::check_points(ecsimd_bls381_g2_check, "ecsimd_bls381_g2_check", "g2_check", in192, 192); }
// (k[i] Q[i], ok) for the 256-bit integers k
inline std::pair<byte_records, mask> g2_mul(byte_records const& k, byte_records const& in192) {
  return detail::mul(ecsimd_bls381_g2_mul, "ecsimd_bls381_g2_mul", "g2_mul", k, in192, 192);
}
// what g2_msm(n terms, bits, alg) will do.  Host only: no context, no GPU.
inline ecsimd_msm_plan_t g2_msm_plan(size_t n, int bits = 255, int alg = ECSIMD_MSM_ALG_AUTO) {
  return detail::msm_plan(ecsimd_bls381_g2_msm_plan, "ecsimd_bls381_g2_msm_plan", n, bits, alg);
}
// a sum across lanes: its 192-byte encoding, whether it is another point than infinity, and how many points were malformed (and contributed nothing)
struct g2_sum_result { std::vector<uint8_t> encoding; bool finite; uint32_t invalid; };
// the sum of (k[i] mod 2^bits) Q[i]
inline g2_sum_result g2_msm(byte_records const& k, byte_records const& pts192, int bits = 255, int alg = ECSIMD_MSM_ALG_AUTO) {
  return detail::msm<g2_sum_result>(ecsimd_bls381_g2_msm, "ecsimd_bls381_g2_msm", "g2_msm", k, pts192, 192, bits, alg);
}
// the sum of the points: records of 192 bytes, or of 96 (compressed; the width decides)
inline g2_sum_result g2_point_sum(byte_records const& pts) {
  return detail::point_sum<g2_sum_result>(ecsimd_bls381_g2_point_sum, "ecsimd_bls381_g2_point_sum", "g2_point_sum", pts, 192, ECSIMD_BLS381_G2_UNCOMPRESSED,
                                          ECSIMD_BLS381_G2_COMPRESSED);
}
}  // namespace bls12_381
}  // namespace hip
}  // namespace ecsimd
#endif
