// ecsimd/sm2.h -- the SM2 signature scheme on the device (GB/T 32918.2; not in the reference): hip::sm3 and hip::sm2_za / sm2_digest / sm2_pubkey /
// sm2_verify / sm2_verify_digest / sm2_sign_digest over ecsimd_sm2.h, templated on the Curve -- curve_sm2 (ecsimd/curve_sm2.h), or any Curve that names its
// group order N and has the ECDSA capability.  Integers are wide_bignum<bignum_256>, public keys wide_curve_point<Curve>; digests (Z_A, e) are the integers
// whose 32 big-endian bytes the hash is.  Private keys and nonces are SECRET (what that means on the device: ecsimd_sm2.h).
#ifndef ECSIMD_SM2_CPP_H
#define ECSIMD_SM2_CPP_H
#include <ecsimd/curve_point.h>
#include <ecsimd/sha256.h>
#include <ecsimd_sm2.h>
#include <string>
#include <utility>

namespace ecsimd {
namespace hip {
// The signers' identities: one for the whole batch (the standard's default "1234567812345678" where none is given), or one per lane, all of one length
class sm2_identity {
 public:
  sm2_identity() : sm2_identity(std::string("1234567812345678")) {}
  explicit sm2_identity(std::string const& shared) : rows_(reinterpret_cast<const uint8_t*>(shared.data()), 1, shared.size(), shared.size()), stride_(0) {}
  explicit sm2_identity(messages per_lane) : rows_(std::move(per_lane)), stride_(rows_.size() > 1 ? rows_.stride_bytes() : 0), per_lane_(true) {}
  const uint8_t* data() const { return rows_.data(); }
  size_t id_bytes() const { return rows_.msg_bytes(); }
  size_t id_stride() const { return stride_; }
  void fits(size_t n, const char* what) const { if (per_lane_ && rows_.size() != n) throw error(std::string("ecsimd: ") + what + ": one identity per lane, or one for the batch"); }
 private:
  messages rows_;
  size_t stride_;
  bool per_lane_ = false;
};
namespace detail {
inline void sm2_same(size_t a, size_t b, const char* what) { if (a != b) throw error(std::string("ecsimd: ") + what + ": operands disagree on the batch"); }
inline const uint32_t* sm2_lens(messages const& m, const lengths* lens, const char* what) {
  if (lens) sm2_same(lens->size(), m.size(), what);
  return lens ? lens->data() : nullptr;
}
}  // namespace detail
using sm2_bn = wide_bignum<bignum_256>;

// e[i] = SM3(message i) as an integer; lens: one length per lane (hip::ragged)
inline sm2_bn sm3(messages const& m, const lengths* lens = nullptr) {
  auto e = sm2_bn::uninitialized(m.size());
  check(ecsimd_sm2_sm3(context(), m.data(), m.msg_bytes(), m.stride_bytes(), detail::sm2_lens(m, lens, "sm3"), e.data(), m.size()), "ecsimd_sm2_sm3");
  return e;
}
// Z_A of each public key under its identity
template <class Curve> sm2_bn sm2_za(wide_curve_point<Curve> const& Q, sm2_identity const& id = sm2_identity()) {
  id.fits(Q.size(), "sm2_za");
  auto za = sm2_bn::uninitialized(Q.size());
  check(ecsimd_sm2_za(context(), hip_curve_id_of<Curve>(), Q.x().data(), Q.y().data(), id.data(), id.id_bytes(), id.id_stride(), za.data(), Q.size()), "ecsimd_sm2_za");
  return za;
}
// e = SM3(Z_A || M)
template <class Curve> sm2_bn sm2_digest(wide_curve_point<Curve> const& Q, messages const& m, sm2_identity const& id = sm2_identity(), const lengths* lens = nullptr) {
  id.fits(Q.size(), "sm2_digest"); detail::sm2_same(m.size(), Q.size(), "sm2_digest");
  auto e = sm2_bn::uninitialized(Q.size());
  check(ecsimd_sm2_digest(context(), hip_curve_id_of<Curve>(), Q.x().data(), Q.y().data(), id.data(), id.id_bytes(), id.id_stride(), m.data(), m.msg_bytes(), m.stride_bytes(),
                          detail::sm2_lens(m, lens, "sm2_digest"), e.data(), Q.size()), "ecsimd_sm2_digest");
  return e;
}
// d G for the SECRET keys; ok is 0, and the point (0, 0), where d is not in [1, n - 2]
template <class Curve> wide_curve_point<Curve> sm2_pubkey(sm2_bn const& d, mask& ok) {
  auto x = sm2_bn::uninitialized(d.size()), y = sm2_bn::uninitialized(d.size());
  ok = mask(d.size());
  check(ecsimd_sm2_pubkey(context(), hip_curve_id_of<Curve>(), d.data(), x.data(), y.data(), ok.data(), d.size()), "ecsimd_sm2_pubkey");
  return wide_curve_point<Curve>(std::move(x), std::move(y));
}
// one byte per lane: 1 where (r, s) is accepted for the digest e under Q
template <class Curve> mask sm2_verify_digest(sm2_bn const& e, sm2_bn const& r, sm2_bn const& s, wide_curve_point<Curve> const& Q) {
  detail::sm2_same(e.size(), Q.size(), "sm2_verify_digest"); detail::sm2_same(r.size(), Q.size(), "sm2_verify_digest"); detail::sm2_same(s.size(), Q.size(), "sm2_verify_digest");
  mask ok(Q.size());
  check(ecsimd_sm2_verify_digest(context(), hip_curve_id_of<Curve>(), e.data(), r.data(), s.data(), Q.x().data(), Q.y().data(), ok.data(), Q.size()), "ecsimd_sm2_verify_digest");
  return ok;
}
// ... for the message under Q and its identity
template <class Curve> mask sm2_verify(wide_curve_point<Curve> const& Q, messages const& m, sm2_bn const& r, sm2_bn const& s, sm2_identity const& id = sm2_identity(),
                                       const lengths* lens = nullptr) {
  id.fits(Q.size(), "sm2_verify"); detail::sm2_same(m.size(), Q.size(), "sm2_verify"); detail::sm2_same(r.size(), Q.size(), "sm2_verify"); detail::sm2_same(s.size(), Q.size(), "sm2_verify");
  mask ok(Q.size());
  check(ecsimd_sm2_verify(context(), hip_curve_id_of<Curve>(), Q.x().data(), Q.y().data(), id.data(), id.id_bytes(), id.id_stride(), m.data(), m.msg_bytes(), m.stride_bytes(),
                          detail::sm2_lens(m, lens, "sm2_verify"), r.data(), s.data(), ok.data(), Q.size()), "ecsimd_sm2_verify");
  return ok;
}
// (r, s) for the digests e under the SECRET keys d and nonces *k; k == nullptr: the deterministic nonce (ecsimd_sm2.h says which, and that SM2 has no
// standard one).  ok is 0, and r = s = 0, where the rule set refuses the lane.
template <class Curve> std::pair<sm2_bn, sm2_bn> sm2_sign_digest(sm2_bn const& e, sm2_bn const& d, const sm2_bn* k, mask& ok) {
  detail::sm2_same(e.size(), d.size(), "sm2_sign_digest");
  if (k) detail::sm2_same(k->size(), d.size(), "sm2_sign_digest");
  auto r = sm2_bn::uninitialized(d.size()), s = sm2_bn::uninitialized(d.size());
  ok = mask(d.size());
  check(ecsimd_sm2_sign_digest(context(), hip_curve_id_of<Curve>(), e.data(), d.data(), k ? k->data() : nullptr, r.data(), s.data(), ok.data(), d.size(), 0), "ecsimd_sm2_sign_digest");
  return {r, s};
}
}  // namespace hip
}  // namespace ecsimd
#endif
