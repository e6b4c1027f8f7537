// ecsimd/msm.h -- multi-scalar multiplication on the device: hip::msm<Curve> (R = sum k_i P_i by the bucket method), hip::point_sum<Curve> and hip::msm_plan
// over ecsimd_msm.h (not in the reference).  Scalars are a wide_bignum<bignum_256>, points a wide_curve_point<Curve> (affine classical, (0, 0) the point at
// infinity); the result is ONE point.  PUBLIC data only (what that means on the device: ecsimd_msm.h).  Curve: curve_nist_p256 or curve_secp256k1.
#ifndef ECSIMD_MSM_CPP_H
#define ECSIMD_MSM_CPP_H
#include <ecsimd/curve_group.h>
#include <ecsimd_msm.h>
#include <optional>

namespace ecsimd {
namespace hip {
// One affine point, or none: the sum was the point at infinity.  invalid = the input points that failed validation and were left out.
struct msm_result {
  std::optional<std::pair<bignum_256, bignum_256>> point;
  uint32_t invalid = 0;
  bool finite() const { return point.has_value(); }
};
namespace detail {
struct msm_out {
  wide_bignum<bignum_256> x = wide_bignum<bignum_256>::uninitialized(1), y = wide_bignum<bignum_256>::uninitialized(1);
  mask finite{1};
  buffer invalid{2};
  msm_result host() const {
    msm_result r;
    uint64_t w[2] = {0, 0}; invalid.download(w);
    r.invalid = (uint32_t)w[0];
    if (finite.get(0)) r.point = std::make_pair(x.get(0), y.get(0));
    return r;
  }
};
}  // namespace detail

// what msm(n terms, bits, alg) will do: the route, c, the windows, L, m, the serial bound, the launches and the workspace.  Host only: no context, no GPU.
inline ecsimd_msm_plan_t msm_plan(size_t n, int bits = 256, int alg = ECSIMD_MSM_ALG_AUTO) {
  ecsimd_msm_plan_t p;
  if (ecsimd_msm_plan(n, bits, alg, &p) != ECSIMD_HIP_OK) throw error("ecsimd_msm_plan: bits must be 1 .. 256, n at most 2^24, alg AUTO, BUCKETS or LANES");
  return p;
}
// sum over i of (k[i] mod 2^bits) P[i]
template <class Curve>
msm_result msm(wide_bignum<bignum_256> const& k, wide_curve_point<Curve> const& P, int bits = 256, int alg = ECSIMD_MSM_ALG_AUTO) {
  if (k.size() != P.size()) throw error("ecsimd: msm: one scalar per point");
  detail::msm_out o;
  check(ecsimd_msm(context(), curve_group<Curve>::curve_id(), k.data(), P.x().data(), P.y().data(), o.x.data(), o.y.data(), o.finite.data(),
                   reinterpret_cast<uint32_t*>(o.invalid.data()), k.size(), bits, alg), "ecsimd_msm");
  return o.host();
}
// sum over i of P[i]
template <class Curve>
msm_result point_sum(wide_curve_point<Curve> const& P) {
  detail::msm_out o;
  check(ecsimd_msm_point_sum(context(), curve_group<Curve>::curve_id(), P.x().data(), P.y().data(), o.x.data(), o.y.data(), o.finite.data(),
                             reinterpret_cast<uint32_t*>(o.invalid.data()), P.size()), "ecsimd_msm_point_sum");
  return o.host();
}
}  // namespace hip
}  // namespace ecsimd
#endif
