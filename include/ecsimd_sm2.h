/* ecsimd_sm2.h -- the SM2 signature scheme (GB/T 32918.2-2016, ISO/IEC 14888-3:2018; RFC 8998's sm2sig_sm3) on the device: the SM3 hash (GB/T 32905-2016),
 * the identity digest Z_A, public keys, verification and signing.
 *
 * The functions live in libecsimd_hip.so beside those of ecsimd_hip.h and take the same context: its stream, its workspace and its error string
 * (ecsimd_hip_last_error).  They return ECSIMD_HIP_OK or an ECSIMD_HIP_ERR_* code.  Plain C99.
 *
 * THE CURVE is a curve registered at run time (ecsimd_hip_register_curve) that has the ECSIMD_HIP_CURVE_ECDSA capability: its order n >= 2^255 and p < 2n.
 * ecsimd_sm2_curve registers sm2p256v1, the curve the standard recommends (GB/T 32918.5); any other such curve is taken as well -- Z_A hashes the curve's own
 * a, b and G.  The built-in ids ECSIMD_HIP_P256 and ECSIMD_HIP_SECP256K1 are refused (register the curve with ECSIMD_HIP_CURVE_GENERIC_KERNELS if SM2 over
 * one of them is what you want), and so is a context with ECSIMD_HIP_REF_SQUARE_COMPAT set, as the ECDSA calls refuse it.  The point arithmetic is the
 * registered curve's: the constant-time comb for secret scalars, the combs and the window loop of ecsimd_hip_double_scalar_mult for public ones.
 *
 * Integers cross as the ECDSA calls take them: n x 4 little-endian 64-bit limbs, 16-byte aligned device memory.  A digest -- Z_A, e, the output of sm3 --
 * is the integer whose 32 big-endian bytes the hash is, as ecsimd_hip_sha256 writes its digests.  Messages are addressed as ecsimd_hip_sha256_lens's: lane
 * i's bytes at msg + i * stride_bytes, msg_bytes of them, or lens[i] (at most stride_bytes; lens 4-byte aligned) where lens is not NULL; no byte behind a
 * message is read; a message is shorter than 2^31 bytes.  Identities: lane i's at id + i * id_stride, id_bytes of them (the same length in the whole batch,
 * at most 8191: ENTL has 16 bits); id_stride = 0 is one ID for the whole batch.  The standard's default ID is the 16 bytes "1234567812345678".
 *
 * THE RULES (GB/T 32918.2 clauses 6 and 7), with t = (r + s) mod n:
 *     Z_A    = SM3(ENTL || ID || a || b || x_G || y_G || x_A || y_A),   e = SM3(Z_A || M)
 *     verify = 1 <= r < n  and  1 <= s < n  and  t != 0  and  Q is on the curve with x, y < p (the point (0, 0) is not)  and  R = s G + t Q is finite
 *              and  (e mod n + x(R) mod n) mod n == r.          e is ANY 256-bit value; x(R) >= n is reduced.  There is no modular inversion.
 *     sign   : r = (e + x(k G)) mod n,  s = (1 + d)^-1 (k - r d) mod n;
 *              ok = 1 <= d <= n - 2  and  1 <= k <= n - 1  and  r != 0  and  r + k != n  and  s != 0;   r = s = 0 where not ok: a new nonce is the caller's.
 *     pubkey : ok = 1 <= d <= n - 2 (d = n - 1 has no signature: 1 + d is not invertible), the point is (0, 0) where not.
 *
 * Common to all calls but ecsimd_sm2_curve: stream-ordered, nothing is read back; n = 0 succeeds; a NULL array with n > 0 is refused
 * (ECSIMD_HIP_ERR_BAD_ARG), and so is an output that is one of the inputs or another output.  pubkey, verify_digest, verify and sign_digest use the context
 * WORKSPACE and the curve's window tables: a call can be captured into a graph once the same call has run at the same n and the same lengths outside a
 * capture; one that would have to grow the workspace under capture returns ECSIMD_HIP_ERR_BAD_ARG ("the context workspace would have to grow during stream
 * capture ...") BEFORE it touches the stream, so the capture stays valid.  sm3, za and digest use neither.
 *
 * SECRETS.  In pubkey and sign_digest the private key d, the nonce k, the HMAC state behind a deterministic nonce, 1 + d, its inverse, k - r d and every
 * point on the way to the result are secret: no branch condition, address or lane mask in force at a memory access depends on them (one exception, RFC 6979's
 * own: "this candidate was out of range", see ecsimd_hip_rfc6979_nonce), `ok` is written by selects, and the SM2 kernels that see them use no scratch memory.
 * Only n and the curve are public.  Both calls zero what they used of the workspace before they return, whatever their launches said.  sm3, za, digest,
 * verify_digest and verify take public data only.
 */
#ifndef ECSIMD_SM2_H
#define ECSIMD_SM2_H
#include "ecsimd_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* *curve_id = the id of sm2p256v1 (GB/T 32918.5; RFC 8998), registered on the first call; the same id on every later call and in every thread.  Host only:
 * no context, no device work.  The id is what curves.curve_id("sm2") and ecsimd_hip_register_curve with the same parameters return. */
int ecsimd_sm2_curve(int* curve_id);

/* e = SM3 of each lane's message.  lens may be NULL (every lane has msg_bytes bytes). */
int ecsimd_sm2_sm3(ecsimd_hip_ctx* ctx, const uint8_t* msg, size_t msg_bytes, size_t stride_bytes, const uint32_t* lens, uint64_t* e, size_t n);

/* za = Z_A of each lane's public key (qx, qy) and identity.  The key is hashed as it is given (32 bytes per coordinate), NOT validated: verify does that. */
int ecsimd_sm2_za(ecsimd_hip_ctx* ctx, int curve, const uint64_t* qx, const uint64_t* qy, const uint8_t* id, size_t id_bytes, size_t id_stride, uint64_t* za, size_t n);

/* e = SM3(Z_A || M): Z_A is made in registers and never written. */
int ecsimd_sm2_digest(ecsimd_hip_ctx* ctx, int curve, const uint64_t* qx, const uint64_t* qy, const uint8_t* id, size_t id_bytes, size_t id_stride, const uint8_t* msg,
                      size_t msg_bytes, size_t stride_bytes, const uint32_t* lens, uint64_t* e, size_t n);

/* (qx, qy) = d G for the SECRET d: the constant-time comb.  ok[i] = 1 iff 1 <= d <= n - 2; (0, 0) where not.  At most 2^22 keys per call. */
int ecsimd_sm2_pubkey(ecsimd_hip_ctx* ctx, int curve, const uint64_t* d, uint64_t* qx, uint64_t* qy, uint8_t* ok, size_t n);

/* ok[i] = the verdict of the rule above on the digest e, the signature (r, s) and the public key (qx, qy).  Public data only. */
int ecsimd_sm2_verify_digest(ecsimd_hip_ctx* ctx, int curve, const uint64_t* e, const uint64_t* r, const uint64_t* s, const uint64_t* qx, const uint64_t* qy, uint8_t* ok,
                             size_t n);

/* The same from the message: ecsimd_sm2_digest into the workspace, then ecsimd_sm2_verify_digest's launches -- the same kernels, one call. */
int ecsimd_sm2_verify(ecsimd_hip_ctx* ctx, int curve, const uint64_t* qx, const uint64_t* qy, const uint8_t* id, size_t id_bytes, size_t id_stride, const uint8_t* msg,
                      size_t msg_bytes, size_t stride_bytes, const uint32_t* lens, const uint64_t* r, const uint64_t* s, uint8_t* ok, size_t n);

/* (r, s) for the digest e under the SECRET key d and the SECRET nonce k.  flags must be 0.  At most 2^22 signatures per call.
 * k == NULL: a DETERMINISTIC nonce, made in the workspace and never returned.  SM2 HAS NO STANDARD DETERMINISTIC NONCE: this one is ecsimd_hip_rfc6979_nonce's
 * (RFC 6979 3.2 with HMAC-SHA-256 over d and e as given, qlen = 256, at most C(n) candidates -- 4 for sm2p256v1), a choice of this library.  The signature
 * is an ordinary SM2 signature: ANY verifier accepts it, and nothing about the choice can be seen from outside.  A lane that exhausts the candidates
 * (probability below 2^-128) gets ok = 0.
 * There is no message-level call: ecsimd_sm2_digest, then this one, is the chain. */
int ecsimd_sm2_sign_digest(ecsimd_hip_ctx* ctx, int curve, const uint64_t* e, const uint64_t* d, const uint64_t* k, uint64_t* r, uint64_t* s, uint8_t* ok, size_t n, int flags);

#ifdef __cplusplus
}
#endif
#endif
