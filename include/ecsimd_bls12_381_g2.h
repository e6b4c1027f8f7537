/* ecsimd_bls12_381_g2.h -- BLS12-381 G2 on the device: the standard encodings, validation and the subgroup test, per-lane scalar products, the multi-scalar
 * multiplication R = sum k_i Q_i by the bucket method, and the sum of a batch of points (signature aggregation in the min-pubkey variant).  The G1 calls are in
 * ecsimd_bls12_381.h; these are their twins with the widths changed, under the prefix ecsimd_bls381_g2_.
 *
 * The functions live in libecsimd_hip.so beside those of ecsimd_hip.h and take the same context: its stream, its grow-only workspace and its error string
 * (ecsimd_hip_last_error).  They return ECSIMD_HIP_OK or an ECSIMD_HIP_ERR_* code.  Plain C99.
 *
 * THE CURVE.  Fp2 = Fp[u] / (u^2 + 1) over the 381-bit prime p of ecsimd_bls12_381.h; E': y^2 = x^3 + 4 (1 + u) over Fp2; G2 is its subgroup of the 255-bit
 * prime order r = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001.  #E'(Fp2) = h2 r with a 507-bit cofactor h2: MOST POINTS OF E'(Fp2) ARE
 * NOT IN G2 -- a random point of the curve is in G2 with probability 2^-507.
 *
 * WIRE FORMATS: the ZCash / IETF BLS serialisation.  An Fp2 coordinate c0 + c1 u is written c1 FIRST.
 *   Uncompressed, 192 bytes: x.c1 || x.c0 || y.c1 || y.c0, 48 big-endian bytes each, the top three bits of byte 0 zero.  Infinity is 0x40 and 191 zero bytes.
 *   Compressed, 96 bytes: x.c1 || x.c0, with bit 7 of byte 0 set; bit 6 = infinity (then every other bit is 0: 0xc0 and 95 zero bytes); bit 5 = y is the
 *   lexicographically largest of the two roots: y.c1 > (p - 1) / 2, or y.c1 = 0 and y.c0 > (p - 1) / 2.
 *   ANYTHING ELSE IS MALFORMED, never "fixed up": any of the four components >= p, wrong flag bits (the sort bit together with infinity included), a non-zero
 *   byte anywhere behind an infinity flag, an x whose x^3 + 4 (1 + u) has no root in Fp2, a point not on E'.
 * Byte arrays lie in device memory, n records one behind the other, at ANY alignment (word accesses where an array's base is a multiple of 4, byte accesses
 * otherwise, decided per array).  SCALARS for _mul and _msm are n x 4 x uint64_t little-endian limbs, 16-byte aligned: exactly ecsimd_msm's `k`.
 *
 * VALIDATION is ON-CURVE ONLY everywhere except _check: decoding a point proves it lies on E', not that it lies in G2.  A caller that needs membership calls
 * ecsimd_bls381_g2_check.  Every sum and product here is defined over the INTEGERS (k Q for the integer k), so a point outside G2 still has a well-defined answer.
 *
 * PUBLIC DATA ONLY.  Nothing here is constant-time: validity, every exceptional case of the group law and every scalar bit is a branch, and the bucket
 * method's memory addresses are scalar digits.  Not for secret scalars.
 *
 * Common to all calls: stream-ordered, nothing is read back; n = 0 succeeds; a NULL array with n > 0 is refused (ECSIMD_HIP_ERR_BAD_ARG), and so is an output
 * that overlaps an input or another output.  decompress, compress, check, mul and raw use no workspace.  _msm and _point_sum use the context WORKSPACE
 * (_msm_plan's workspace_bytes; 288 bytes per 16 points plus 16 for the point sum).  CAPTURE: they only enqueue kernels and can be captured into a graph after
 * ONE warm-up call at the same (n, bits, flags) on the same context; a call that would have to grow the workspace while the stream is being captured returns
 * ECSIMD_HIP_ERR_BAD_ARG with "capture" in the message BEFORE it touches the stream, so the capture stays valid.  Contexts with ECSIMD_HIP_REF_SQUARE_COMPAT set
 * are accepted and compute the same bytes.
 */
#ifndef ECSIMD_BLS12_381_G2_H
#define ECSIMD_BLS12_381_G2_H
#include "ecsimd_msm.h"

#ifdef __cplusplus
extern "C" {
#endif

/* out192[i] = the uncompressed form of the compressed in96[i]; ok[i] = 1.  A malformed lane gets 192 zero bytes and ok = 0.  On-curve only. */
int ecsimd_bls381_g2_decompress(ecsimd_hip_ctx* ctx, const uint8_t* in96, uint8_t* out192, uint8_t* ok, size_t n);

/* out96[i] = the compressed form of the uncompressed in192[i], validated the same way; a malformed lane gets 96 zero bytes and ok = 0. */
int ecsimd_bls381_g2_compress(ecsimd_hip_ctx* ctx, const uint8_t* in192, uint8_t* out96, uint8_t* ok, size_t n);

/* on_curve[i] = in192[i] decodes (infinity does); in_subgroup[i] = it decodes AND [r] Q is the identity -- the definition, computed as such (255 doublings and
 * the additions of r's set bits per lane).  Infinity is on the curve and in the subgroup; a malformed lane is neither. */
int ecsimd_bls381_g2_check(ecsimd_hip_ctx* ctx, const uint8_t* in192, uint8_t* on_curve, uint8_t* in_subgroup, size_t n);

/* out192[i] = k[i] Q[i] for the 256-bit INTEGER k[i] (not reduced modulo r: the same point where Q is in G2, and well defined where it is not) and the
 * validated Q[i]; ok[i] = 1.  Left-to-right double-and-add with mixed additions.  A malformed lane gets 192 zero bytes and ok = 0. */
int ecsimd_bls381_g2_mul(ecsimd_hip_ctx* ctx, const uint64_t* k, const uint8_t* in192, uint8_t* out192, uint8_t* ok, size_t n);

/* Where AUTO changes route: the measured crossover at bits = 255 -- the power of two from which BUCKETS stays ahead of LANES by more than the repeat spread --
 * from ONE run of tools/time_bls12_381_g2.py, routes alternating, one MI355X (profiles/r22/bls12_381_g2.txt; that run was made while this constant still held
 * G1's 2^18, and AUTO is never timed).  There BUCKETS takes 45.5 ms against LANES' 90.9 at 2^17 terms, 79.6 against 171.8 at 2^18, 61.7 against 335.4 at 2^19
 * and 68.9 against 661.0 at 2^20; at 2^16 LANES wins, 50.0 ms against 53.0 (BUCKETS' slowest repeat 56.0, fastest 52.0: clear of LANES' 49.9 .. 50.3).  As on G1
 * the crossing is NOT clean below: at 2^12 both routes are latency and BUCKETS is the faster one, 26.4 ms against 43.9 (LANES is one lane's 512 dependent point
 * operations, which do not get cheaper with fewer lanes): a caller with a small sum who minds the difference asks for BUCKETS itself.  One step lower than G1's
 * 2^18: the per-lane product grew by 4.1 to 4.9 times against G1's, the bucket route by 3.0 to 3.2. */
#define ECSIMD_BLS381_G2_MSM_AUTO_THRESHOLD ((size_t)1 << 17)

/* R = sum over i < n of (k[i] mod 2^bits) Q[i], as 192 bytes at out192, with finite[0] = 1 (0 and the infinity encoding where R is the identity).  bits in
 * 1 .. 256: only the low `bits` bits of each scalar are read.  n <= ECSIMD_MSM_MAX_N.  `flags` is ecsimd_msm's route, same values and meaning:
 * ECSIMD_MSM_ALG_AUTO (LANES below ECSIMD_BLS381_G2_MSM_AUTO_THRESHOLD terms, BUCKETS from there on), ECSIMD_MSM_ALG_BUCKETS (the bucket method of ecsimd_msm.h
 * on this group), ECSIMD_MSM_ALG_LANES (per-lane products as _mul computes them, then the tree sum): all routes give the same bytes.  Points are validated
 * ON-CURVE but NOT for subgroup membership.  A malformed point contributes nothing and is counted in invalid[0] (one uint32_t, 4-byte aligned; may be NULL);
 * infinity contributes nothing and is not counted.  The INTERNAL CHECK rule of ecsimd_msm.h applies unchanged: should the sort's invariants fail, out192 is 192
 * bytes of 0xff, finite[0] = 1 and invalid[0] = UINT32_MAX.  SCHEDULE and CAPTURE as ecsimd_msm: a function of (n, bits, flags) only; _msm_plan reports it. */
int ecsimd_bls381_g2_msm(ecsimd_hip_ctx* ctx, const uint64_t* k, const uint8_t* pts192, uint8_t* out192, uint8_t* finite, uint32_t* invalid, size_t n, int bits,
                         int flags);

/* `flags` of _point_sum */
enum { ECSIMD_BLS381_G2_UNCOMPRESSED = 0, ECSIMD_BLS381_G2_COMPRESSED = 1 };
/* R = sum over i < n of Q[i]: the tree sum behind the validating front, lanes owning strided slices of 16 points, one launch per level.  pts is n x 192 bytes,
 * or n x 96 with ECSIMD_BLS381_G2_COMPRESSED (signatures arrive compressed: each lane then pays one square root in Fp2).  Any n up to 2^31 x 16 points;
 * out192, finite and invalid as _msm's; malformed points are counted and skipped.  Launches: 3 + max(0, ceil(log16 n) - 1); n = 0: 1. */
int ecsimd_bls381_g2_point_sum(ecsimd_hip_ctx* ctx, const uint8_t* pts, uint8_t* out192, uint8_t* finite, uint32_t* invalid, size_t n, int flags);

/* Host only: no context, no GPU.  What _msm will do for (n, bits, flags): the BUCKETS schedule is the same function of (n, bits) as ecsimd_msm_plan's and
 * ecsimd_bls12_381_g1_msm_plan's (c, windows, buckets, L, m, max_chain and launches are equal) with this group's 96-byte elements in workspace_bytes; LANES is
 * 3 + the tree's passes launches and 16 + 288 n bytes, max_chain = 16.  ECSIMD_HIP_ERR_BAD_ARG for bits outside 1 .. 256, n > ECSIMD_MSM_MAX_N, a flag that is
 * no route, or out == NULL. */
int ecsimd_bls381_g2_msm_plan(size_t n, int bits, int flags, ecsimd_msm_plan_t* out);

/* Diagnostic, as ecsimd_bls12_381_raw is: ONE function of the layers below on raw operands, for tests.  A record is 48 big-endian bytes; lane i reads
 * ecsimd_bls381_g2_raw_inputs(op) records at in + 48 * inputs * i and writes ecsimd_bls381_g2_raw_outputs(op) records at out + 48 * outputs * i.  An Fp2 operand
 * is TWO records, c0 THEN c1 -- NOT the wire order, which has c1 first.  ALL 2^384 values of a component are accepted as the residue they are congruent to;
 * results are canonical plain residues.  A flag record is 1 or 0 in its last byte.  A point operand is x (two records), y (two records) and a flag "this is the
 * identity" (x and y ignored then); a point result likewise (x = y = 0 at the identity).  Points are NOT validated.  Public data only.
 *     op  name         in                          out
 *      0  FE2_MUL      a, b                        a b
 *      1  FE2_SQR      a                           a^2
 *      2  FE2_ADD      a, b                        a + b
 *      3  FE2_SUB      a, b                        a - b
 *      4  FE2_NEG      a                           -a
 *      5  FE2_INVERT   a                           1 / a (0 -> 0)
 *      6  FE2_SQRT     a                           a candidate root, flag "its square is a" (a root is returned whenever one exists)
 *      7  FE2_CANON    a                           a, both components reduced
 *      8  POINT_ADD    x1, y1, id1, x2, y2, id2    the Jacobian sum, every exceptional pair decided
 *      9  POINT_DBL    x, y, id                    the double
 *     10  POINT_MADD   x1, y1, id1, x2, y2         the mixed sum (the second operand finite and affine) */
enum { ECSIMD_BLS381_G2_RAW_FE2_MUL = 0, ECSIMD_BLS381_G2_RAW_FE2_SQR = 1, ECSIMD_BLS381_G2_RAW_FE2_ADD = 2, ECSIMD_BLS381_G2_RAW_FE2_SUB = 3,
       ECSIMD_BLS381_G2_RAW_FE2_NEG = 4, ECSIMD_BLS381_G2_RAW_FE2_INVERT = 5, ECSIMD_BLS381_G2_RAW_FE2_SQRT = 6, ECSIMD_BLS381_G2_RAW_FE2_CANON = 7,
       ECSIMD_BLS381_G2_RAW_POINT_ADD = 8, ECSIMD_BLS381_G2_RAW_POINT_DBL = 9, ECSIMD_BLS381_G2_RAW_POINT_MADD = 10 };
int ecsimd_bls381_g2_raw(ecsimd_hip_ctx* ctx, int op, const uint8_t* in, uint8_t* out, size_t n);
int ecsimd_bls381_g2_raw_inputs(int op);   /* records per lane; 0 for an unknown op */
int ecsimd_bls381_g2_raw_outputs(int op);

#ifdef __cplusplus
}
#endif
#endif
