// ecsimd/ntt.h -- the number-theoretic transform on the device: hip::ntt::domain (RAII over ecsimd_ntt_domain), forward, inverse, bitrev and plan over
// ecsimd_ntt.h (not in the reference).  An array is a wide_bignum<bignum_256> of batch * n lanes, batch arrays of n = 2^log_n elements one after the other:
// classical values in, canonical classical values out.  PUBLIC OR SECRET-INDEPENDENT: the schedule is a function of the sizes alone (ecsimd_ntt.h).
#ifndef ECSIMD_NTT_CPP_H
#define ECSIMD_NTT_CPP_H
#include <ecsimd/bignum.h>
#include <ecsimd_ntt.h>
#include <string>
#include <utility>

namespace ecsimd {
namespace hip {
namespace ntt {
struct field_info { int two_adicity; bignum_256 root; };
// the two-adicity and the default root of a prime field id.  Host only.
inline field_info info(int field) {
  field_info f;
  if (ecsimd_ntt_field_info(field, &f.two_adicity, f.root.limbs.data()) != ECSIMD_HIP_OK) throw error("ecsimd_ntt_field_info: the field must be a modulus registered as prime");
  return f;
}
// BLS12-381's scalar field: its field id and the conventional root 7^((r - 1) / 2^32).  Host only.
inline std::pair<int, bignum_256> bls12_381_fr() {
  int field = -1; bignum_256 root;
  if (ecsimd_ntt_bls12_381_fr(&field, root.limbs.data()) != ECSIMD_HIP_OK) throw error("ecsimd_ntt_bls12_381_fr failed");
  return {field, root};
}
// what a transform of `batch` arrays of 2^log_n elements will do.  Host only.
inline ecsimd_ntt_plan_t plan(int log_n, size_t batch = 1, int flags = 0) {
  ecsimd_ntt_plan_t p;
  if (ecsimd_ntt_plan(log_n, batch, flags, &p) != ECSIMD_HIP_OK) throw error("ecsimd_ntt_plan: log_n must be 1 .. 24, batch at least 1, flags 0 or ECSIMD_NTT_MAX_RADIX_LOG(1 .. 9)");
  return p;
}

// The domain {shift w^k} of size 2^log_n: the subgroup for shift == nullptr, the field's default root for root == nullptr.
class domain {
 public:
  domain(int field, int log_n, bignum_256 const* root = nullptr, bignum_256 const* shift = nullptr) : field_(field), log_n_(log_n) {
    check(ecsimd_ntt_domain_create(context(), field, log_n, root ? root->limbs.data() : nullptr, shift ? shift->limbs.data() : nullptr, &dom_), "ecsimd_ntt_domain_create");
  }
  domain(domain const&) = delete;
  domain& operator=(domain const&) = delete;
  domain(domain&& o) noexcept : field_(o.field_), log_n_(o.log_n_), dom_(std::exchange(o.dom_, nullptr)) {}
  domain& operator=(domain&& o) noexcept {
    if (this != &o) { reset(); field_ = o.field_; log_n_ = o.log_n_; dom_ = std::exchange(o.dom_, nullptr); }
    return *this;
  }
  ~domain() { reset(); }
  int field() const { return field_; }
  int log_n() const { return log_n_; }
  size_t size() const { return (size_t)1 << log_n_; }
  ecsimd_ntt_domain const* get() const { return dom_; }

 private:
  void reset() { if (dom_) { (void)ecsimd_ntt_domain_destroy(context(), dom_); dom_ = nullptr; } }
  int field_, log_n_;
  ecsimd_ntt_domain* dom_ = nullptr;
};

namespace detail {
inline size_t batch_of(size_t lanes, size_t n, const char* what) {
  if (lanes % n) throw error(std::string("ecsimd: ") + what + ": the lanes are no whole number of arrays");
  return lanes / n;
}
}  // namespace detail
// out[k] = sum over i of x[i] (shift w^k)^i in each array
inline wide_bignum<bignum_256> forward(domain const& d, wide_bignum<bignum_256> const& x, int flags = 0) {
  auto out = wide_bignum<bignum_256>::uninitialized(x.size());
  check(ecsimd_ntt_forward(context(), d.get(), x.data(), out.data(), detail::batch_of(x.size(), d.size(), "ntt::forward"), flags), "ecsimd_ntt_forward");
  return out;
}
// the exact inverse of forward on the same domain
inline wide_bignum<bignum_256> inverse(domain const& d, wide_bignum<bignum_256> const& x, int flags = 0) {
  auto out = wide_bignum<bignum_256>::uninitialized(x.size());
  check(ecsimd_ntt_inverse(context(), d.get(), x.data(), out.data(), detail::batch_of(x.size(), d.size(), "ntt::inverse"), flags), "ecsimd_ntt_inverse");
  return out;
}
// out[rev(i)] = x[i] in each array of 2^log_n lanes
inline wide_bignum<bignum_256> bitrev(int log_n, wide_bignum<bignum_256> const& x) {
  if (log_n < 1 || log_n > ECSIMD_NTT_MAX_LOG_N) throw error("ecsimd: ntt::bitrev: log_n must be 1 .. 24");
  auto out = wide_bignum<bignum_256>::uninitialized(x.size());
  check(ecsimd_ntt_bitrev(context(), log_n, x.data(), out.data(), detail::batch_of(x.size(), (size_t)1 << log_n, "ntt::bitrev")), "ecsimd_ntt_bitrev");
  return out;
}
}  // namespace ntt
}  // namespace hip
}  // namespace ecsimd
#endif
