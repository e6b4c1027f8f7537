// ecsimd/curve_sm2.h -- sm2p256v1, the curve GB/T 32918.5-2017 recommends for the SM2 algorithms (RFC 8998 "curveSM2"): y^2 = x^3 - 3x + b over GF(p).
// Member names follow the reference's curve struct (curve_nist_p256.h:14-32): bn_type, P, A, B, Gx, Gy, each with a ::value; N, the group order, is what
// gives the curve its comb, double_scalar_mult, ECDSA and the SM2 signature scheme (ecsimd/sm2.h).  The curve runs on the generic kernels; the engine's id
// of it (hip_curve_id_of<curve_sm2>()) is the one ecsimd_sm2_curve returns -- tests/cpp/sm2_tests.cpp holds the two together.
#ifndef ECSIMD_CURVE_SM2_H
#define ECSIMD_CURVE_SM2_H
#include <ecsimd/curve.h>

namespace ecsimd {
struct curve_sm2 {
  using bn_type = bignum_256;
  using P  = bn256_constant<0xfffffffeffffffffull, 0xffffffffffffffffull, 0xffffffff00000000ull, 0xffffffffffffffffull>;   // 2^256 - 2^224 - 2^96 + 2^64 - 1
  using A  = bn256_constant<0xfffffffeffffffffull, 0xffffffffffffffffull, 0xffffffff00000000ull, 0xfffffffffffffffcull>;   // p - 3
  using B  = bn256_constant<0x28e9fa9e9d9f5e34ull, 0x4d5a9e4bcf6509a7ull, 0xf39789f515ab8f92ull, 0xddbcbd414d940e93ull>;
  using Gx = bn256_constant<0x32c4ae2c1f198119ull, 0x5f9904466a39c994ull, 0x8fe30bbff2660be1ull, 0x715a4589334c74c7ull>;
  using Gy = bn256_constant<0xbc3736a2f4f6779cull, 0x59bdcee36b692153ull, 0xd0a9877cc62a4740ull, 0x02df32e52139f0a0ull>;
  using N  = bn256_constant<0xfffffffeffffffffull, 0xffffffffffffffffull, 0x7203df6b21c6052bull, 0x53bbf40939d54123ull>;
};
}  // namespace ecsimd
#endif
