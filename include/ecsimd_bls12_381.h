/* ecsimd_bls12_381.h -- BLS12-381 G1 on the device: the standard encodings, validation and the subgroup test, per-lane scalar products, the multi-scalar
 * multiplication R = sum k_i P_i by the bucket method, and the sum of a batch of points (public-key aggregation).
 *
 * The functions live in libecsimd_hip.so beside those of ecsimd_hip.h and take the same context: its stream, its grow-only workspace and its error string
 * (ecsimd_hip_last_error).  They return ECSIMD_HIP_OK or an ECSIMD_HIP_ERR_* code.  Plain C99.
 *
 * THE CURVE.  E: y^2 = x^3 + 4 over GF(p), p the 381-bit prime 0x1a0111ea397fe69a4b1ba7b6434bacd764774b84f38512bf6730d2a0f6b0f6241eabfffeb153ffffb9feffffffffaaab;
 * G1 is its subgroup of the 255-bit prime order r = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001.  #E(Fp) = h r with a 126-bit cofactor
 * h: most points of E(Fp) are NOT in G1.
 *
 * WIRE FORMATS: the ZCash / IETF BLS serialisation.
 *   Uncompressed, 96 bytes: x || y, 48 big-endian bytes each, the top three bits of byte 0 zero.  Infinity is 0x40 followed by 95 zero bytes.
 *   Compressed, 48 bytes: x, with bit 7 of byte 0 set; bit 6 = infinity (then every other bit is 0: 0xc0 and 47 zero bytes); bit 5 = y is the
 *   lexicographically largest of the two roots (y > (p - 1) / 2).
 *   ANYTHING ELSE IS MALFORMED, never "fixed up": a coordinate >= p, wrong flag bits, a non-zero body behind the infinity flag, an x with no square root, a
 *   point not on the curve.
 * Byte arrays lie in device memory, n records one behind the other, at ANY alignment (word accesses where an array's base is a multiple of 4, byte accesses
 * otherwise, decided per array).  SCALARS for g1_mul and g1_msm are n x 4 x uint64_t little-endian limbs, 16-byte aligned: exactly ecsimd_msm's `k`, so the
 * shared stages of the bucket method read them unchanged (the Python Engine converts from bytes).
 *
 * VALIDATION is ON-CURVE ONLY everywhere except g1_check: decoding a point proves it lies on E, not that it lies in G1.  A caller that needs membership calls
 * ecsimd_bls12_381_g1_check.  Every sum and product here is defined over the INTEGERS (k P for the integer k), so a point outside G1 still has a well-defined answer.
 *
 * PUBLIC DATA ONLY.  Nothing here is constant-time: validity, every exceptional case of the group law and every scalar bit is a branch, and the bucket
 * method's memory addresses are scalar digits.  Not for secret scalars.
 *
 * Common to all calls: stream-ordered, nothing is read back; n = 0 succeeds; a NULL array with n > 0 is refused (ECSIMD_HIP_ERR_BAD_ARG), and so is an output
 * that overlaps an input or another output.  decompress, compress, check, mul and raw use no workspace.  g1_msm and g1_point_sum use the context WORKSPACE
 * (g1_msm_plan's workspace_bytes; 144 bytes per 16 points plus 16 for the point sum).  CAPTURE: they only enqueue kernels and can be captured into a graph
 * after ONE warm-up call at the same (n, bits, flags) on the same context; a call that would have to grow the workspace while the stream is being captured
 * returns ECSIMD_HIP_ERR_BAD_ARG with "capture" in the message BEFORE it touches the stream, so the capture stays valid.  Contexts with
 * ECSIMD_HIP_REF_SQUARE_COMPAT set are accepted and compute the same bytes.
 */
#ifndef ECSIMD_BLS12_381_H
#define ECSIMD_BLS12_381_H
#include "ecsimd_msm.h"

#ifdef __cplusplus
extern "C" {
#endif

/* out96[i] = the uncompressed form of the compressed in48[i]; ok[i] = 1.  A malformed lane gets 96 zero bytes and ok = 0.  On-curve only. */
int ecsimd_bls12_381_g1_decompress(ecsimd_hip_ctx* ctx, const uint8_t* in48, uint8_t* out96, uint8_t* ok, size_t n);

/* out48[i] = the compressed form of the uncompressed in96[i], validated the same way; a malformed lane gets 48 zero bytes and ok = 0. */
int ecsimd_bls12_381_g1_compress(ecsimd_hip_ctx* ctx, const uint8_t* in96, uint8_t* out48, uint8_t* ok, size_t n);

/* on_curve[i] = in96[i] decodes (infinity does); in_subgroup[i] = it decodes AND [r] P is the identity -- the definition, computed as such (255 doublings and
 * the additions of r's set bits per lane).  Infinity is on the curve and in the subgroup; a malformed lane is neither. */
int ecsimd_bls12_381_g1_check(ecsimd_hip_ctx* ctx, const uint8_t* in96, uint8_t* on_curve, uint8_t* in_subgroup, size_t n);

/* out96[i] = k[i] P[i] for the 256-bit INTEGER k[i] (not reduced modulo r: the same point where P is in G1, and well defined where it is not) and the
 * validated P[i]; ok[i] = 1.  Left-to-right double-and-add with mixed additions.  A malformed lane gets 96 zero bytes and ok = 0. */
int ecsimd_bls12_381_g1_mul(ecsimd_hip_ctx* ctx, const uint64_t* k, const uint8_t* in96, uint8_t* out96, uint8_t* ok, size_t n);

/* Where AUTO changes route: the measured crossover at bits = 255 -- from where on BUCKETS stays ahead by more than the repeat spread --, rounded up to a power
 * of two (tools/time_bls12_381.py, one MI355X, profiles/r21/bls12_381.txt).  There BUCKETS takes 27.4 ms against LANES' 38.2 at 2^18 terms, 23.2 against 135.5
 * at 2^20 and 44.3 against 525.6 at 2^22; at 2^16 LANES wins, 14.0 ms against 17.0; 2^17 was not timed.  The crossing is NOT clean below: at 2^8 .. 2^14 both
 * routes are latency (LANES 12.3 - 13.1 ms, one lane's 512 dependent point operations; BUCKETS 9.0 - 11.6 ms, its chain of launches), and BUCKETS is the
 * faster one by 1.1 - 1.4 times: a caller with a 4096-term sum who minds the 3 ms asks for BUCKETS itself. */
#define ECSIMD_BLS12_381_MSM_AUTO_THRESHOLD ((size_t)1 << 18)

/* R = sum over i < n of (k[i] mod 2^bits) P[i], as 96 bytes at out96, with finite[0] = 1 (0 and the infinity encoding where R is the identity).  bits in
 * 1 .. 256: only the low `bits` bits of each scalar are read.  n <= ECSIMD_MSM_MAX_N.  `flags` is ecsimd_msm's route, same values and meaning:
 * ECSIMD_MSM_ALG_AUTO (LANES below ECSIMD_BLS12_381_MSM_AUTO_THRESHOLD terms, BUCKETS from there on), ECSIMD_MSM_ALG_BUCKETS (the bucket method of ecsimd_msm.h
 * on this group: one mixed Jacobian addition per term and window, the shared sort, reduction and tree), ECSIMD_MSM_ALG_LANES (per-lane products as g1_mul
 * computes them, then the tree sum): all routes give the same bytes.  Points are validated ON-CURVE but NOT for subgroup membership (see
 * ecsimd_bls12_381_g1_check).  A malformed point contributes nothing and is counted in invalid[0] (one uint32_t, 4-byte aligned; may be NULL); infinity
 * contributes nothing and is not counted.  The INTERNAL CHECK rule of ecsimd_msm.h applies unchanged: should the sort's invariants fail, out96 is 96 bytes of
 * 0xff, finite[0] = 1 and invalid[0] = UINT32_MAX.  SCHEDULE and CAPTURE as ecsimd_msm: a function of (n, bits, flags) only; g1_msm_plan reports it. */
int ecsimd_bls12_381_g1_msm(ecsimd_hip_ctx* ctx, const uint64_t* k, const uint8_t* pts96, uint8_t* out96, uint8_t* finite, uint32_t* invalid, size_t n, int bits,
                            int flags);

/* `flags` of g1_point_sum */
enum { ECSIMD_BLS12_381_UNCOMPRESSED = 0, ECSIMD_BLS12_381_COMPRESSED = 1 };
/* R = sum over i < n of P[i]: the tree sum behind the validating front, lanes owning strided slices of 16 points, one launch per level.  pts is n x 96 bytes,
 * or n x 48 with ECSIMD_BLS12_381_COMPRESSED (public keys arrive compressed: each lane then pays one square root).  Any n up to 2^31 x 16 points; out96,
 * finite and invalid as g1_msm's; malformed points are counted and skipped.  Launches: 3 + max(0, ceil(log16 n) - 1); n = 0: 1. */
int ecsimd_bls12_381_g1_point_sum(ecsimd_hip_ctx* ctx, const uint8_t* pts, uint8_t* out96, uint8_t* finite, uint32_t* invalid, size_t n, int flags);

/* Host only: no context, no GPU.  What g1_msm will do for (n, bits, flags), as ecsimd_msm_plan reports it for ecsimd_msm: the BUCKETS schedule is the same
 * function of (n, bits) (c, windows, buckets, L, m, max_chain and launches are equal) with this group's 48-byte field elements in workspace_bytes; LANES is
 * 3 + the tree's passes launches and 16 + 144 n bytes, max_chain = 16 (the per-lane product's 512 operations are its own).  ECSIMD_HIP_ERR_BAD_ARG for bits
 * outside 1 .. 256, n > ECSIMD_MSM_MAX_N, a flag that is no route, or out == NULL. */
int ecsimd_bls12_381_g1_msm_plan(size_t n, int bits, int flags, ecsimd_msm_plan_t* out);

/* Diagnostic, as ecsimd_p384_raw is: ONE function of the layers below on raw operands, for tests.  A record is 48 big-endian bytes; lane i reads
 * ecsimd_bls12_381_raw_inputs(op) records at in + 48 * inputs * i and writes ecsimd_bls12_381_raw_outputs(op) records at out + 48 * outputs * i.  Field operands:
 * ALL 2^384 values are accepted as the residue they are congruent to (the layer works on canonical Montgomery-form values; the conversion at the door takes any
 * 384-bit value); results are canonical plain residues.  A flag record is 1 or 0 in its last byte.  A point operand is x, y and a flag "this is the identity"
 * (x and y ignored then); a point result likewise (x = y = 0 at the identity).  Points are NOT validated.  Public data only.
 *     op  name         in                          out
 *      0  FE_MUL       a, b                        a b mod p
 *      1  FE_SQR       a                           a^2
 *      2  FE_ADD       a, b                        a + b
 *      3  FE_SUB       a, b                        a - b
 *      4  FE_NEG       a                           -a
 *      5  FE_INVERT    a                           a^(p - 2) (0 -> 0)
 *      6  FE_SQRT      a                           a^((p + 1) / 4), flag "its square is a"
 *      7  FE_CANON     a                           a mod p
 *      8  POINT_ADD    x1, y1, id1, x2, y2, id2    the Jacobian sum, every exceptional pair decided
 *      9  POINT_DBL    x, y, id                    the double
 *     10  POINT_MADD   x1, y1, id1, x2, y2         the mixed sum (the second operand finite and affine) */
enum { ECSIMD_BLS12_381_RAW_FE_MUL = 0, ECSIMD_BLS12_381_RAW_FE_SQR = 1, ECSIMD_BLS12_381_RAW_FE_ADD = 2, ECSIMD_BLS12_381_RAW_FE_SUB = 3, ECSIMD_BLS12_381_RAW_FE_NEG = 4,
       ECSIMD_BLS12_381_RAW_FE_INVERT = 5, ECSIMD_BLS12_381_RAW_FE_SQRT = 6, ECSIMD_BLS12_381_RAW_FE_CANON = 7, ECSIMD_BLS12_381_RAW_POINT_ADD = 8,
       ECSIMD_BLS12_381_RAW_POINT_DBL = 9, ECSIMD_BLS12_381_RAW_POINT_MADD = 10 };
int ecsimd_bls12_381_raw(ecsimd_hip_ctx* ctx, int op, const uint8_t* in, uint8_t* out, size_t n);
int ecsimd_bls12_381_raw_inputs(int op);   /* records per lane; 0 for an unknown op */
int ecsimd_bls12_381_raw_outputs(int op);

#ifdef __cplusplus
}
#endif
#endif
