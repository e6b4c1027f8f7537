/* ecsimd_p384.h -- NIST P-384 (secp384r1; FIPS 186-4 D.1.2.4) on the device: SHA-384, public keys, ECDH, ECDSA verification and deterministic ECDSA signing.
 *
 * The functions live in libecsimd_hip.so beside those of ecsimd_hip.h and take the same context: its stream, its workspace and its error string
 * (ecsimd_hip_last_error).  They return ECSIMD_HIP_OK or an ECSIMD_HIP_ERR_* code.  Plain C99.
 *
 * Integers cross as 48 big-endian bytes, as SEC 1 and FIPS 186 write them: a private key d, a digest, a shared secret z.  A public key is X || Y, 96 bytes
 * (no 0x04 in front, no compression); a signature is r || s, 96 bytes (no DER).  Every array lies in device memory, n records one behind the other, at any
 * alignment: word accesses where an array's base is a multiple of 4, byte accesses otherwise, decided per array.
 *
 * `digest` is the 48-byte string bits2int sees (RFC 6979 2.3.2 with qlen = 384): SHA-384 output as it is; a shorter hash is left-padded with zero bytes by
 * the caller.  e is that integer, reduced modulo the group order n where it is used.
 *
 * Common to all calls: stream-ordered, nothing is read back; n = 0 succeeds; a NULL array with n > 0 is refused (ECSIMD_HIP_ERR_BAD_ARG), and so is an output
 * that is one of the inputs or another output.  A call walks its batch in chunks of 2^16 lanes per launch.  ecdh, ecdsa_verify, ecdsa_sign and the raw
 * multiplications use the context WORKSPACE (1152 bytes per lane of a chunk for the lanes' tables; 52 for signing's nonce): a call can be captured into a
 * graph once the same call has run at the same or a larger n outside a capture; one that would have to grow the workspace under capture returns
 * ECSIMD_HIP_ERR_BAD_ARG ("the context workspace would have to grow during stream capture ...") BEFORE it touches the stream, so the capture stays valid.
 * sha384 and pubkey use no workspace.  Contexts with ECSIMD_HIP_REF_SQUARE_COMPAT set are ACCEPTED and compute the same bytes: none of the reference's
 * arithmetic is involved.
 *
 * The group law is the complete one of Renes, Costello and Batina (2016) for a = -3 in homogeneous projective coordinates: there are no exceptional inputs.
 * Decoding a point validates it: x, y < p and y^2 = x^3 - 3 x + b.  The cofactor is 1, so that is full validation.
 *
 * SECRETS.  In pubkey, ecdh and ecdsa_sign the private key d, the nonce k, the HMAC states K and V, e + r d and every point on the way to the result are
 * secret: no branch condition, address or lane mask in force at a memory access depends on them, nothing is declassified, `ok` is written by selects, and
 * the kernels use no scratch memory.  Only n, lengths and strides are public.  ecdsa_sign wipes its workspace (k and its validity) before it returns,
 * whatever its launches said; ecdh's workspace holds multiples of the PUBLIC peer only.  sha384, ecdsa_verify and raw take public data only.
 */
#ifndef ECSIMD_P384_H
#define ECSIMD_P384_H
#include "ecsimd_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* digest = SHA-384 (FIPS 180-4) of each lane's message, n x 48 bytes.  Messages are addressed as ecsimd_hip_sha512's and ecsimd_ed25519_sign's: lane i's
 * bytes at msg + i * stride_bytes, msg_bytes of them, or lens[i] (at most stride_bytes; lens 4-byte aligned) where lens is not NULL. */
int ecsimd_p384_sha384(ecsimd_hip_ctx* ctx, const uint8_t* msg, size_t msg_bytes, size_t stride_bytes, const uint32_t* lens, uint8_t* digest, size_t n);

/* pub = d G for the SECRET d (n x 48): a constant-time comb over committed multiples of G.  ok[i] = 1 iff 1 <= d < n; pub[i] is 96 zero bytes where not. */
int ecsimd_p384_pubkey(ecsimd_hip_ctx* ctx, const uint8_t* d, uint8_t* pub, uint8_t* ok, size_t n);

/* z = x(d peer) for the SECRET d and the peer's public key (n x 96), n x 48 bytes: a fixed signed 4-bit window loop over the lane's own table.
 * ok[i] = 1 iff 1 <= d < n and peer[i] decodes; z[i] is 48 zero bytes where not.  (d peer is never the identity for such inputs: the order is prime.) */
int ecsimd_p384_ecdh(ecsimd_hip_ctx* ctx, const uint8_t* d, const uint8_t* peer, uint8_t* z, uint8_t* ok, size_t n);

/* ok[i] = 1 iff ALL of: 1 <= r, s < n; pub[i] decodes; R = u1 G + u2 Q with u1 = e / s, u2 = r / s modulo n is not the identity; x(R) mod n = r.
 * The last test is made without leaving projective form (r Z = X, or (r + n) Z = X where r + n < p), so x(R) >= n is handled.  Public data only. */
int ecsimd_p384_ecdsa_verify(ecsimd_hip_ctx* ctx, const uint8_t* pub, const uint8_t* digest, const uint8_t* sig, uint8_t* ok, size_t n);

/* sig = r || s, deterministic ECDSA (RFC 6979 with HMAC-SHA-384; hlen = qlen = 384, so bits2int is the identity on the 48 bytes and bits2octets one
 * conditional subtraction of n) for the SECRET d: k = the FIRST candidate, R = k G, r = x(R) mod n, s = (e + r d) / k mod n.  flags must be 0.
 * DEVIATION FROM RFC 6979: there is no retry.  A candidate is 0 or >= n with probability below 2^-194 (2^384 - n has 190 bits), and by the rule
 * ecsimd_hip_rfc6979_nonce documents one candidate suffices for a failure probability below 2^-128; a lane whose candidate is out of range, or whose r or s
 * comes out 0, gets ok = 0 and 96 zero bytes, as does a lane with d outside [1, n - 1].  No such input is known. */
int ecsimd_p384_ecdsa_sign(ecsimd_hip_ctx* ctx, const uint8_t* d, const uint8_t* digest, uint8_t* sig, uint8_t* ok, size_t n, int flags);

/* Diagnostic, as ecsimd_ed25519_raw is: ONE function of the layers below on raw operands, for tests.  A record is 48 big-endian bytes; lane i reads
 * ecsimd_p384_raw_inputs(op) records at in + 48 * inputs * i and writes ecsimd_p384_raw_outputs(op) records at out + 48 * outputs * i.  Field and scalar
 * operands: ALL 2^384 values are accepted as the residue they are congruent to; results are canonical.  A flag record is 1 or 0 in its last byte.  A point
 * result is x, y and a flag "this is the identity" (x = y = 0 then).  Public data only; at most 2^16 lanes of the multiplications per call.
 *     op  name            in                          out
 *      0  FE_MUL          a, b                        a b mod p
 *      1  FE_SQR          a                           a^2
 *      2  FE_ADD          a, b                        a + b
 *      3  FE_SUB          a, b                        a - b
 *      4  FE_NEG          a                           -a
 *      5  FE_INVERT       a                           a^(p - 2) (0 -> 0)
 *      6  FE_CANON        a                           a mod p
 *      7  SC_MUL          a, b                        a b mod n
 *      8  SC_INVERT       a                           a^(n - 2) mod n (0 -> 0)
 *      9  DECODE_ENCODE   x, y                        x, y, flag "decodes" (x = y = 0 where it does not)
 *     10  POINT_ADD       x1, y1, id1, x2, y2, id2    the sum by Algorithm 4 (id = 1: that operand is the identity, its x and y are ignored)
 *     11  POINT_DBL       x, y, id                    the double by Algorithm 6
 *     12  BASE_MULT       k                           (k mod n) G by the comb of pubkey
 *     13  VAR_MULT        k, x, y                     (k mod n) P by the loop of ecdh
 *     14  DOUBLE_MULT     u1, u2, x, y                (u1 mod n) G + (u2 mod n) Q by the loop of ecdsa_verify
 * Points handed to ops 10 - 14 are NOT validated. */
enum { ECSIMD_P384_RAW_FE_MUL = 0, ECSIMD_P384_RAW_FE_SQR = 1, ECSIMD_P384_RAW_FE_ADD = 2, ECSIMD_P384_RAW_FE_SUB = 3, ECSIMD_P384_RAW_FE_NEG = 4,
       ECSIMD_P384_RAW_FE_INVERT = 5, ECSIMD_P384_RAW_FE_CANON = 6, ECSIMD_P384_RAW_SC_MUL = 7, ECSIMD_P384_RAW_SC_INVERT = 8, ECSIMD_P384_RAW_DECODE_ENCODE = 9,
       ECSIMD_P384_RAW_POINT_ADD = 10, ECSIMD_P384_RAW_POINT_DBL = 11, ECSIMD_P384_RAW_BASE_MULT = 12, ECSIMD_P384_RAW_VAR_MULT = 13, ECSIMD_P384_RAW_DOUBLE_MULT = 14 };
int ecsimd_p384_raw(ecsimd_hip_ctx* ctx, int op, const uint8_t* in, uint8_t* out, size_t n);
int ecsimd_p384_raw_inputs(int op);   /* records per lane; 0 for an unknown op */
int ecsimd_p384_raw_outputs(int op);

#ifdef __cplusplus
}
#endif
#endif
