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
// G1's and G2's calls (ecsimd/bls12_381_g2.h) over the C function `fn`, its name `cname` (the exception's text), the C++ name `what` and the records' widths
template <class Fn> std::pair<byte_records, mask> recode(Fn fn, const char* cname, const char* what, byte_records const& in, size_t in_width, size_t out_width) {
  sizes(in, in.size(), in_width, what);
  byte_records out(in.size(), out_width);
  mask ok(in.size());
  check(fn(context(), in.data(), out.data(), ok.data(), in.size()), cname);
  return {out, ok};
}
template <class Fn> std::pair<mask, mask> check_points(Fn fn, const char* cname, const char* what, byte_records const& in, size_t width) {
  sizes(in, in.size(), width, what);
  mask on(in.size()), sub(in.size());
  check(fn(context(), in.data(), on.data(), sub.data(), in.size()), cname);
  return {on, sub};
}
template <class Fn> std::pair<byte_records, mask> mul(Fn fn, const char* cname, const char* what, byte_records const& k, byte_records const& in, size_t width) {
  sizes(k, in.size(), 32, what);
  sizes(in, in.size(), width, what);
  byte_records out(in.size(), width);
  mask ok(in.size());
  check(fn(context(), limbs(k), in.data(), out.data(), ok.data(), in.size()), cname);
  return {out, ok};
}
template <class Fn> ecsimd_msm_plan_t msm_plan(Fn fn, const char* cname, size_t n, int bits, int alg) {
  ecsimd_msm_plan_t p;
  if (fn(n, bits, alg, &p) != ECSIMD_HIP_OK) throw error(std::string(cname) + ": bits must be 1 .. 256, n at most 2^24, alg AUTO, BUCKETS or LANES");
  return p;
}
// a sum across lanes into Result = {encoding of `width` bytes, finite, invalid}; call(out, finite, invalid) is the C function
template <class Result, class Call> Result sum(Call call, size_t width, const char* cname) {
  byte_records out(1, width), invalid(1, 4);
  mask finite(1);
  check(call(out.data(), finite.data(), reinterpret_cast<uint32_t*>(invalid.data())), cname);
  Result r{out.get(0), finite.get(0) != 0, 0};
  const std::vector<uint8_t> count = invalid.get(0);
  std::memcpy(&r.invalid, count.data(), 4);
  return r;
}
template <class Result, class Fn> Result msm(Fn fn, const char* cname, const char* what, byte_records const& k, byte_records const& pts, size_t width, int bits, int alg) {
  sizes(k, pts.size(), 32, what);
  sizes(pts, pts.size(), width, what);
  return sum<Result>([&](uint8_t* out, uint8_t* finite, uint32_t* invalid) { return fn(context(), limbs(k), pts.data(), out, finite, invalid, pts.size(), bits, alg); }, width, cname);
}
// pts: records of `width` bytes, or of width / 2 (compressed; the width decides between the two flags)
template <class Result, class Fn>
Result point_sum(Fn fn, const char* cname, const char* what, byte_records const& pts, size_t width, int uncompressed_flag, int compressed_flag) {
  if (pts.size() && pts.width() != width && pts.width() != width / 2)
    throw error(std::string("ecsimd: bls12_381::") + what + ": records of " + std::to_string(width) + " or " + std::to_string(width / 2) + " bytes");
  const int flags = pts.width() == width / 2 ? compressed_flag : uncompressed_flag;
  return sum<Result>([&](uint8_t* out, uint8_t* finite, uint32_t* invalid) { return fn(context(), pts.data(), out, finite, invalid, pts.size(), flags); }, width, cname);
}
}  // namespace detail

// (uncompressed points, ok) of the compressed ones; a malformed lane is zeros with ok = 0
inline std::pair<byte_records, mask> g1_decompress(byte_records const& in48) {
  return detail::recode(ecsimd_bls12_381_g1_decompress, "ecsimd_bls12_381_g1_decompress", "g1_decompress", in48, 48, 96);
}
// (compressed points, ok) of the uncompressed ones, validated the same way
inline std::pair<byte_records, mask> g1_compress(byte_records const& in96) {
  return detail::recode(ecsimd_bls12_381_g1_compress, "ecsimd_bls12_381_g1_compress", "g1_compress", in96, 96, 48);
}
// (on the curve, in the subgroup) per lane; the second is [r] P = infinity
inline std::pair<mask, mask> g1_check(byte_records const& in96) { return detail::check_points(ecsimd_bls12_381_g1_check, "ecsimd_bls12_381_g1_check", "g1_check", in96, 96); }
// (k[i] P[i], ok) for the 256-bit integers k
inline std::pair<byte_records, mask> g1_mul(byte_records const& k, byte_records const& in96) {
  return detail::mul(ecsimd_bls12_381_g1_mul, "ecsimd_bls12_381_g1_mul", "g1_mul", k, in96, 96);
}
// what g1_msm(n terms, bits, alg) will do.  Host only: no context, no GPU.
inline ecsimd_msm_plan_t g1_msm_plan(size_t n, int bits = 255, int alg = ECSIMD_MSM_ALG_AUTO) {
  return detail::msm_plan(ecsimd_bls12_381_g1_msm_plan, "ecsimd_bls12_381_g1_msm_plan", n, bits, alg);
}
// a sum across lanes: its 96-byte encoding, whether it is another point than infinity, and how many points were malformed (and contributed nothing)
struct g1_sum_result { std::vector<uint8_t> encoding; bool finite; uint32_t invalid; };
// the sum of (k[i] mod 2^bits) P[i]
inline g1_sum_result g1_msm(byte_records const& k, byte_records const& pts96, int bits = 255, int alg = ECSIMD_MSM_ALG_AUTO) {
  return detail::msm<g1_sum_result>(ecsimd_bls12_381_g1_msm, "ecsimd_bls12_381_g1_msm", "g1_msm", k, pts96, 96, bits, alg);
}
// the sum of the points: records of 96 bytes, or of 48 (compressed; the width decides)
inline g1_sum_result g1_point_sum(byte_records const& pts) {
  return detail::point_sum<g1_sum_result>(ecsimd_bls12_381_g1_point_sum, "ecsimd_bls12_381_g1_point_sum", "g1_point_sum", pts, 96, ECSIMD_BLS12_381_UNCOMPRESSED,
                                          ECSIMD_BLS12_381_COMPRESSED);
}
}  // namespace bls12_381
}  // namespace hip
}  // namespace ecsimd
#endif
