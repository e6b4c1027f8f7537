/* ecsimd_ed25519.h -- Ed25519 (RFC 8032: pure Ed25519, no context, no prehash) on the device: key derivation, signing, verification.
 *
 * The functions live in libecsimd_hip.so beside those of ecsimd_hip.h and take the same context: its stream, its workspace, its error string
 * (ecsimd_hip_last_error).  They return ECSIMD_HIP_OK or an ECSIMD_HIP_ERR_* code.  Plain C99.
 *
 * Ed25519 is a byte format, so keys and signatures cross this boundary as BYTES in device memory, not as limb integers:
 *     seed  n x 32 bytes      the private key as RFC 8032 5.1.5 takes it
 *     pk    n x 32 bytes      the encoding of A: y little-endian in bits 0 .. 254, the parity of x in bit 255
 *     sig   n x 64 bytes      R || s, both little-endian as the RFC writes them
 * at any alignment: word accesses where the array's base is a multiple of 4, byte accesses otherwise.  Messages are addressed exactly as
 * ecsimd_hip_keccak256 addresses them: lane i's message at msg + i * stride_bytes, msg_bytes of it, or lens[i] (never more than stride_bytes) where lens is
 * given (n x uint32, 4-byte aligned; msg_bytes is then ignored); any length including 0; word loads where msg and stride_bytes are multiples of 4; no byte
 * at or behind a lane's message is loaded.  msg may be NULL where no lane has a byte.
 *
 * Common to all four calls: stream-ordered, nothing is read back; n = 0 succeeds; batches go through the workspace in chunks (2^20 lanes for verify, 2^22
 * for the others).  Capturable into a graph once the same call has run at the same (or a larger) batch size outside a capture: the context workspace
 * cannot grow under capture, and a call that would have to grow it returns ECSIMD_HIP_ERR_BAD_ARG ("... during stream capture ...") before it touches the
 * stream, so the capture stays valid.  The multiples of B are constants of the library: no table is built at run time.  Contexts with
 * ECSIMD_HIP_REF_SQUARE_COMPAT set are ACCEPTED and compute the same bytes: none of the reference's arithmetic is involved.
 *
 * SECRETS.  In pubkey and sign the seed, h = SHA-512(seed), a, the prefix, r, both hash states, the products [a]B and [r]B and their inverses are secret
 * until the call returns them: no branch, address or lane mask in force at a memory access depends on them (only message lengths, n and strides are public),
 * nothing is declassified, the kernels use no scratch memory, and every workspace byte the call used is zeroed on the stream before it returns, whatever
 * the launches said.  The public key is always derived from the seed inside the call: no entry point takes a (secret, public) pair, because a mismatched
 * pair leaks the key.
 *
 * VERIFICATION RULES (RFC 8032 5.1.7 with strict decoding and the cofactorless equation).  ok[i] = 1 iff
 *     1. s < L;
 *     2. A decodes: y < p, x^2 = (y^2 - 1) / (d y^2 + 1) has a root, and the encoding is not x = 0 with the sign bit set;
 *     3. the canonical encoding of [s]B - [k]A equals the 32 bytes of R as given, k = SHA-512(R || A || M) mod L over the bytes as given.
 * R is never decompressed: a non-canonical or off-curve R cannot equal a canonical encoding.  With ECSIMD_ED25519_REJECT_SMALL_ORDER a lane whose A or R is
 * one of the eight small-order encodings (01 00..00, ec ff..ff 7f, 00..00, 00..00 80, c7176a70..037a and ..03fa, 26e8958f..fc05 and ..fc85) is refused as
 * well, as `verify_strict` implementations do.  DIFFERENCE FROM libcrypto (checked against OpenSSL 3.0.2): libcrypto accepts some non-canonical A, such as
 * y = p + 1 and 01 00..00 80; this call refuses them.  The cofactored equation (strict encodings; not ZIP-215) is ecsimd_ed25519_batch.h's: ecsimd_ed25519_verify_cofactored() per lane,
 * ecsimd_ed25519_verify_batch() for one verdict per batch with ecsimd_ed25519_batch_plan() and ecsimd_ed25519_batch_randomizers(), on the bucket sum
 * ecsimd_ed25519_msm() / ecsimd_ed25519_msm_plan().  k is reduced modulo L before [k]A, as libcrypto
 * reduces it, and there is no subgroup check: a key (or an R) with a small-order component is accepted or refused by that equation alone, so for
 * A = [a]B + T_A, R = [r]B + T_R, s = r + k a the verdict is whether T_R + [k mod L]T_A is the identity (tests/golden/ed25519_verdicts.json).
 */
#ifndef ECSIMD_ED25519_H
#define ECSIMD_ED25519_H
#include "ecsimd_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { ECSIMD_ED25519_REJECT_SMALL_ORDER = 1 };

/* pk = encode([a]B), a = the clamped low half of SHA-512(seed) (RFC 8032 5.1.5). */
int ecsimd_ed25519_pubkey(ecsimd_hip_ctx* ctx, const uint8_t* seed, uint8_t* pk, size_t n);
/* RFC 8032 5.1.6 bit for bit.  pk (optional output, may be NULL) receives the public key of each seed. */
int ecsimd_ed25519_sign(ecsimd_hip_ctx* ctx, const uint8_t* seed, const uint8_t* msg, size_t msg_bytes, size_t stride_bytes, const uint32_t* lens,
                        uint8_t* sig, uint8_t* pk, size_t n);
/* ok: n bytes, 1 or 0 by the rules above.  flags: 0 or ECSIMD_ED25519_REJECT_SMALL_ORDER.  Public data only: the loop is indexed by the scalars' digits. */
int ecsimd_ed25519_verify(ecsimd_hip_ctx* ctx, const uint8_t* pk, const uint8_t* msg, size_t msg_bytes, size_t stride_bytes, const uint32_t* lens,
                          const uint8_t* sig, uint8_t* ok, size_t n, int flags);

/* Diagnostic, as ecsimd_hip_fe29_raw is: ONE function of the layers below on raw operands, for tests.  A record is 32 bytes, a little-endian 256-bit
 * value; lane i reads ecsimd_ed25519_raw_inputs(op) records at in + 32 * inputs * i and writes ecsimd_ed25519_raw_outputs(op) records at
 * out + 32 * outputs * i.  Field operands: ALL 2^256 values are accepted as they are (a value >= p stands for the residue it is congruent to); field results
 * are canonical, in [0, p).  A second output record is a flag: 1 or 0 in its first byte, zeros behind it; where it is 0 the first record is zero (except
 * for SQRT_RATIO, whose first record is then what the exponentiation left).  Public data only.
 *     op  name            in                     out
 *      0  FE_MUL          a, b                   a b
 *      1  FE_SQR          a                      a^2
 *      2  FE_ADD          a, b                   a + b
 *      3  FE_SUB          a, b                   a - b
 *      4  FE_NEG          a                      -a
 *      5  FE_INVERT       a                      a^(p - 2)  (0 -> 0)
 *      6  FE_CANON        a                      a mod p
 *      7  SQRT_RATIO      u, v                   x, flag: x = sqrt(u / v) (times sqrt(-1) where v x^2 = -u), flag = a root exists
 *      8  DECODE_ENCODE   encoding               encode(decode(e)), flag = it decodes
 *      9  POINT_ADD       encodings of P, Q      encode(P + Q) by the unified addition, flag = both decode
 *     10  POINT_DBL       encoding of P          encode(2 P) by the dedicated doubling, flag
 *     11  SC_REDUCE       lo, hi (512 bits)      (hi 2^256 + lo) mod L
 *     12  BASE_MULT       k (256 bits)           encode([k mod L]B), by the constant-time comb
 *     13  DOUBLE_MULT     s, h, encoding of P    encode([s mod L]B + [h mod L]P), flag = P decodes; by the verification loop */
enum { ECSIMD_ED25519_RAW_FE_MUL = 0, ECSIMD_ED25519_RAW_FE_SQR = 1, ECSIMD_ED25519_RAW_FE_ADD = 2, ECSIMD_ED25519_RAW_FE_SUB = 3, ECSIMD_ED25519_RAW_FE_NEG = 4,
       ECSIMD_ED25519_RAW_FE_INVERT = 5, ECSIMD_ED25519_RAW_FE_CANON = 6, ECSIMD_ED25519_RAW_SQRT_RATIO = 7, ECSIMD_ED25519_RAW_DECODE_ENCODE = 8,
       ECSIMD_ED25519_RAW_POINT_ADD = 9, ECSIMD_ED25519_RAW_POINT_DBL = 10, ECSIMD_ED25519_RAW_SC_REDUCE = 11, ECSIMD_ED25519_RAW_BASE_MULT = 12,
       ECSIMD_ED25519_RAW_DOUBLE_MULT = 13 };
int ecsimd_ed25519_raw(ecsimd_hip_ctx* ctx, int op, const uint8_t* in, uint8_t* out, size_t n);
int ecsimd_ed25519_raw_inputs(int op);   /* records per lane; 0 for an unknown op */
int ecsimd_ed25519_raw_outputs(int op);

#ifdef __cplusplus
}
#endif
#endif
