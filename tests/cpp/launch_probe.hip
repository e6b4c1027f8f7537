// launch_probe.hip -- test-only: extern "C" doors to the launchers of kernels.h that take the group order as an ARGUMENT (words8 order / gmod M), so that
// tests/test_gpu_launch_tails.py can run the library's own code objects with an order of its choosing and with inputs chosen after a digest is known.
//
// Host code only (built with --cuda-host-only): no kernel and no copy of kernel source is in here; what runs on the device is what libecsimd_hip.so holds.
// gmod is gfield.cuh's own struct, filled field by field from the arrays tests/launch_probe.py derives with Python integers (gmod_constants there), so
// its layout is stated in one place.  Every launch goes to the null stream; the caller synchronises.
#include <string.h>

#include "kernels.h"
#include "gfield.cuh"

using namespace ecsimd_hip;
using launch::words8;
typedef const uint64_t* in64;
typedef uint64_t* out64;

namespace {
words8 order_of(const uint32_t* w) {
  words8 o;
  for (int i = 0; i < 8; ++i) o.w[i] = w[i];
  return o;
}
// consts: seven 8-word values in gmod's order (p, R, R^2, -R, R^3, p - 2, (p + 1) / 4); p30: the nine 30-bit limbs; scalars: p^-1 mod 2^30, m', flags
gmod gmod_of(const uint32_t* consts, const int32_t* p30, const uint32_t* scalars) {
  gmod M;
  memset(&M, 0, sizeof M);
  for (int i = 0; i < 8; ++i) {
    M.p[i] = consts[i];
    M.r[i] = consts[8 + i];
    M.rsq[i] = consts[16 + i];
    M.negr[i] = consts[24 + i];
    M.r3[i] = consts[32 + i];
    M.pm2[i] = consts[40 + i];
    M.psqrt[i] = consts[48 + i];
  }
  for (int i = 0; i < 9; ++i) M.p30[i] = p30[i];
  M.pinv30 = scalars[0];
  M.mprime = scalars[1];
  M.flags = scalars[2];
  return M;
}
int done() { return (int)hipGetLastError(); }
}  // namespace

#define GMOD_ARGS const uint32_t* consts, const int32_t* p30, const uint32_t* scalars
#define GMOD gmod_of(consts, p30, scalars)

extern "C" {
int probe_bip32_master(const uint32_t* order, const uint8_t* seed, size_t seed_bytes, size_t stride_bytes, out64 k, out64 c, uint8_t* ok, size_t n) {
  launch::bip32_master(nullptr, order_of(order), seed, seed_bytes, stride_bytes, k, c, ok, n);
  return done();
}
int probe_bip32_ckd_priv(GMOD_ARGS, in64 k_par, in64 c_par, const uint32_t* index, uint32_t index_all, in64 xP, in64 yP, out64 k_child, out64 c_child, uint8_t* ok, size_t n) {
  launch::bip32_ckd_priv(nullptr, GMOD, k_par, c_par, index, index_all, xP, yP, k_child, c_child, ok, n);
  return done();
}
int probe_bip32_ckd_pub_front(const uint32_t* order, in64 qx, in64 qy, in64 c_par, const uint32_t* index, uint32_t index_all, out64 x, out64 y, out64 t, out64 c_child,
                              uint8_t* valid, size_t n) {
  launch::bip32_ckd_pub_front(nullptr, order_of(order), qx, qy, c_par, index, index_all, x, y, t, c_child, valid, n);
  return done();
}
int probe_bip32_ckd_pub_accept(in64 ax, in64 ay, in64 jz, const uint8_t* valid, out64 cx, out64 cy, out64 c_child, uint8_t* ok, size_t n) {
  launch::bip32_ckd_pub_accept(nullptr, ax, ay, jz, valid, cx, cy, c_child, ok, n);
  return done();
}
int probe_schnorr_verify_front(const uint32_t* order, in64 px, in64 r, in64 s, const uint8_t* msg, size_t msg_bytes, size_t stride_bytes, out64 u1, out64 u2, out64 x, out64 y,
                               uint8_t* valid, size_t n) {
  launch::schnorr_verify_front(nullptr, order_of(order), px, r, s, msg, msg_bytes, stride_bytes, u1, u2, x, y, valid, n);
  return done();
}
int probe_schnorr_nonce(const uint32_t* order, in64 d, in64 aux, in64 px, in64 py, const uint8_t* msg, size_t msg_bytes, size_t stride_bytes, out64 k0, size_t n) {
  launch::schnorr_nonce(nullptr, order_of(order), d, aux, px, py, msg, msg_bytes, stride_bytes, k0, n);
  return done();
}
int probe_schnorr_finish(GMOD_ARGS, in64 d, in64 k0, in64 xP, in64 yP, in64 xR, in64 yR, const uint8_t* msg, size_t msg_bytes, size_t stride_bytes, out64 px, out64 r, out64 s,
                         uint8_t* ok, size_t n) {
  launch::schnorr_finish(nullptr, GMOD, d, k0, xP, yP, xR, yR, msg, msg_bytes, stride_bytes, px, r, s, ok, n);
  return done();
}
int probe_tweak_front(const uint32_t* order, int mode, in64 px, in64 t_or_merkle, out64 x, out64 y, out64 tt, uint8_t* valid, size_t n) {
  launch::tweak_front(nullptr, order_of(order), mode, px, t_or_merkle, x, y, tt, valid, n);
  return done();
}
int probe_taproot_seckey(GMOD_ARGS, in64 d, in64 merkle, in64 xP, in64 yP, out64 d_out, out64 px, uint8_t* ok, size_t n) {
  launch::taproot_seckey(nullptr, GMOD, d, merkle, xP, yP, d_out, px, ok, n);
  return done();
}
int probe_sign_recovery_id(const uint32_t* order, in64 x, in64 y, out64 s, const uint8_t* ok, uint8_t* v, size_t n, int low_s) {
  launch::sign_recovery_id(nullptr, order_of(order), x, y, s, ok, v, n, low_s != 0);
  return done();
}
int probe_ecdsa_sign_scalars(GMOD_ARGS, in64 e, in64 d, in64 k, in64 x, out64 r, out64 s, uint8_t* ok, size_t n) {
  launch::ecdsa_sign_scalars(nullptr, GMOD, e, d, k, x, r, s, ok, n);
  return done();
}
int probe_x_mod_n_equals(int curve, in64 x, const uint8_t* finite, in64 r, uint8_t* ok, size_t n) {
  launch::x_mod_n_equals(nullptr, curve, x, finite, r, ok, n);
  return done();
}
int probe_gc_x_mod_n_equals(GMOD_ARGS, in64 x, const uint8_t* finite, in64 r, uint8_t* ok, size_t n) {
  launch::gc_x_mod_n_equals(nullptr, GMOD, x, finite, r, ok, n);
  return done();
}
}  // extern "C"
