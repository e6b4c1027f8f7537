/* ecsimd_x25519.h -- X25519 (RFC 7748) on the device: key agreement, public keys, and the conversion of Ed25519 keys to X25519 keys.
 *
 * The functions live in libecsimd_hip.so beside those of ecsimd_hip.h and ecsimd_ed25519.h and take the same context: its stream and its error string
 * (ecsimd_hip_last_error).  They return ECSIMD_HIP_OK or an ECSIMD_HIP_ERR_* code.  Plain C99.
 *
 * Scalars, u-coordinates, shared secrets, Ed25519 seeds and Ed25519 public keys are 32-byte little-endian records in device memory, n x 32 bytes per array,
 * at any alignment: word accesses where an array's base is a multiple of 4, byte accesses otherwise, decided per array.
 *
 * Common to all five calls: stream-ordered, nothing is read back; n = 0 succeeds; an output must not be one of the inputs or another output, and a NULL array
 * with n > 0 is refused (ECSIMD_HIP_ERR_BAD_ARG; `ok` of ecsimd_x25519 alone may be NULL).  NO call uses the context workspace: there is nothing to wipe,
 * and every call can be captured into a graph without a warm-up.  A call walks its batch in chunks of 2^20 lanes per launch.  Contexts with
 * ECSIMD_HIP_REF_SQUARE_COMPAT set are ACCEPTED and compute the same bytes: none of the reference's arithmetic is involved.
 *
 * SECRETS.  In ecsimd_x25519 and ecsimd_x25519_base the scalar, every value of the ladder or the comb and the output, and in
 * ecsimd_x25519_from_ed25519_seed the seed, the hash state and the output, are secret until the call returns them: no branch condition, address or lane mask
 * in force at a memory access depends on them, nothing is declassified, and the kernels use neither scratch memory nor LDS.  The peer's u is public by
 * protocol; the kernel nevertheless treats it as it treats the scalar.  ecsimd_x25519_from_ed25519_pk and ecsimd_x25519_raw take public data only.
 */
#ifndef ECSIMD_X25519_H
#define ECSIMD_X25519_H
#include "ecsimd_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* out = X25519(scalar, u), RFC 7748 section 5: the scalar is clamped (bits 0 - 2 and 255 cleared, bit 254 set); bit 255 of u is ignored; a non-canonical u
 * (2^255 - 19 .. 2^255 - 1) is accepted as the residue it stands for; 255 steps of the Montgomery ladder with a24 = 121665; out is the canonical
 * x-coordinate, or 32 zero bytes at infinity.  ok (n bytes, may be NULL): ok[i] = 1 iff out[i] is not all zero -- the check of RFC 7748 section 6.1, made
 * by an OR over the output's words, not by a branch.  DIFFERENCE FROM libcrypto: EVP_PKEY_derive FAILS for the u of small order (0, 1, the bytes e0eb7a7c3b41b8ae1656e3faf19fc46ada098deb9c32b1fd866205165f49b800
 * and 5f9c95bca3508c24b1d0b1559c83ef5b04445cc4581c8e86d8224eddd09f1157, p - 1, p, p + 1, each with bit 255 clear or set: checked against OpenSSL 3.0.2); this
 * call SUCCEEDS and writes zeros with ok = 0 on exactly those lanes.  A caller that ignores ok has agreed on an all-zero secret. */
int ecsimd_x25519(ecsimd_hip_ctx* ctx, const uint8_t* scalar, const uint8_t* u, uint8_t* out, uint8_t* ok, size_t n);

/* out = X25519(scalar, 9), the public key of a private key: bit for bit what ecsimd_x25519 gives on u = 09 00 .. 00, by another route -- the clamped scalar
 * reduced modulo the group order L, the constant-time comb of ecsimd_ed25519_pubkey over the multiples of the Edwards base point B, and the map
 * u = (Z + Y) / (Z - Y).  A clamped scalar is never a multiple of L (8 L > 2^255), so the result is never the point at infinity. */
int ecsimd_x25519_base(ecsimd_hip_ctx* ctx, const uint8_t* scalar, uint8_t* out, size_t n);

/* u = (1 + y) / (1 - y), the X25519 public key of an Ed25519 public key (the sign of x is dropped: a key and its negative give the same u).  ok (n bytes,
 * required): ok[i] = 1 iff pk[i] decodes by the strict rules of ecsimd_ed25519_verify (y < p, a root exists, not x = 0 with the sign bit set) and is none of
 * the eight small-order encodings listed in ecsimd_ed25519.h; u[i] is 32 zero bytes where ok[i] = 0.  Public data only.  There is NO prime-subgroup check:
 * a key with a small-order component is converted.  libsodium's crypto_sign_ed25519_pk_to_curve25519 makes that check and refuses such keys. */
int ecsimd_x25519_from_ed25519_pk(ecsimd_hip_ctx* ctx, const uint8_t* pk, uint8_t* u, uint8_t* ok, size_t n);

/* scalar = the clamped low half of SHA-512(seed): the X25519 private key of an Ed25519 seed, the integer ecsimd_ed25519_pubkey multiplies B by, and what
 * libsodium's crypto_sign_ed25519_sk_to_curve25519 returns.  ecsimd_x25519_base of it is ecsimd_x25519_from_ed25519_pk of the seed's Ed25519 public key. */
int ecsimd_x25519_from_ed25519_seed(ecsimd_hip_ctx* ctx, const uint8_t* seed, uint8_t* scalar, size_t n);

/* Diagnostic, as ecsimd_ed25519_raw is: ONE function of the layers below on raw operands, for tests.  A record is 32 bytes, a little-endian 256-bit value;
 * lane i reads ecsimd_x25519_raw_inputs(op) records at in + 32 * inputs * i and writes ecsimd_x25519_raw_outputs(op) records at out + 32 * outputs * i.
 * Field operands: ALL 2^256 values are accepted as they are; field results are canonical.  A second output record is a flag: 1 or 0 in its first byte,
 * zeros behind it.  Public data only.
 *     op  name            in                     out
 *      0  FE_MUL_SMALL    a                      121665 a mod p
 *      1  LADDER          k, u                   the x-coordinate of [k mod 2^255] u, 0 at infinity: NO clamping, u any 256-bit representative; the device
 *                                                function of ecsimd_x25519
 *      2  ED_TO_MONT      encoding               u, flag: the device function of ecsimd_x25519_from_ed25519_pk */
enum { ECSIMD_X25519_RAW_FE_MUL_SMALL = 0, ECSIMD_X25519_RAW_LADDER = 1, ECSIMD_X25519_RAW_ED_TO_MONT = 2 };
int ecsimd_x25519_raw(ecsimd_hip_ctx* ctx, int op, const uint8_t* in, uint8_t* out, size_t n);
int ecsimd_x25519_raw_inputs(int op);   /* records per lane; 0 for an unknown op */
int ecsimd_x25519_raw_outputs(int op);

#ifdef __cplusplus
}
#endif
#endif
