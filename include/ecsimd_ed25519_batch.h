/* ecsimd_ed25519_batch.h -- Ed25519 batch verification on the device: ONE verdict for a batch of signatures, the per-lane rule that names the culprit in a
 * refused batch, and the multi-scalar multiplication on the twisted Edwards curve both stand on.
 *
 * The functions live in libecsimd_hip.so beside those of ecsimd_ed25519.h and ecsimd_msm.h and take the same context: its stream, its grow-only workspace and
 * its error string (ecsimd_hip_last_error).  They return ECSIMD_HIP_OK or an ECSIMD_HIP_ERR_* code.  Plain C99.
 *
 * OPERANDS, as ecsimd_ed25519_verify takes them: device pointers to BYTES -- pk n x 32, sig n x 64 (R || s), at any alignment; lane i's message at
 * msg + i * stride_bytes, msg_bytes of it or lens[i] (never more than stride_bytes) where lens is given.  PUBLIC DATA ONLY: bucket addresses are scalar
 * digits and the per-lane loop is indexed by them.  Contexts with ECSIMD_HIP_REF_SQUARE_COMPAT set are ACCEPTED, as in ecsimd_ed25519.h.
 *
 * THE RULE (strict encodings with the COFACTORED equation).  A lane passes iff
 *     1. s < L;
 *     2. A AND R decode strictly: y < p, x^2 = (y^2 - 1) / (d y^2 + 1) has a root, and the encoding is not x = 0 with the sign bit set;
 *     3. [8]([s]B - [h]A - R) is the identity, h = SHA-512(R || A || M) mod L over the bytes as given.
 * With ECSIMD_ED25519_REJECT_SMALL_ORDER a lane whose A or R is one of the eight small-order encodings is refused as well, as in ecsimd_ed25519_verify.
 * THIS IS NOT ZIP-215: ZIP-215 also accepts non-canonical encodings of A and R (y >= p), which rule 2 refuses.  Every lane ecsimd_ed25519_verify accepts passes
 * this rule too (multiply its equation by 8); the converse fails for keys or R with a small-order component: of the 1 019 records of
 * tests/golden/ed25519_verdicts.json, 676 pass this rule alone (452 of kind "small order", 224 of the three "mixed ..." kinds), none the cofactorless one alone.
 * Why a batch needs this rule: for a key or an R with a small-order component the randomized COFACTORLESS sum accepts or refuses depending on the randomizers;
 * multiplied by 8 the torsion is gone and the verdict is a function of the batch.
 *
 * THE BATCH METHOD (tools/ed25519_batch_model.py is the normative statement, on hashlib and big integers).  H_tag(x) = SHA256(SHA256(tag) || SHA256(tag) || x):
 *     D_i    = SHA-512(R_i || A_i || M_i), all 64 bytes;  h_i = int(D_i, little-endian) mod L
 *     leaf_i = H_"ecsimd/ed25519-batch/leaf"(D_i || s_i)           (s_i: its 32 bytes as given)
 *     node   = H_"ecsimd/ed25519-batch/node"(c_0 || ... || c_{k-1}), k <= 16 children in lane order, level by level until one digest, the root, remains
 *     seed   = H_"ecsimd/ed25519-batch/seed"(root || n as 8 big-endian bytes);  n = 1: the root is leaf_0
 *     z_i    = (int(H_"ecsimd/ed25519-batch/a"(seed || i as 8 big-endian bytes), big-endian) mod 2^128) | 1
 * A MALFORMED lane -- s_i >= L, A_i or R_i does not decode, or small-order with the flag -- refuses the batch.  Otherwise it is accepted iff
 *     [8]( sum z_i R_i  +  [ sum (z_i h_i mod L) A_i + (L - sum z_i s_i mod L) B ] )  =  the identity:
 * two bucket sums on the Edwards curve (128-bit scalars over n terms, 253-bit scalars over n + 1 terms), one kernel that adds them, doubles three times and
 * tests X = 0 and Y = Z.  No inversion.
 * DETERMINISM.  The seed is a hash of every input: the caller supplies no entropy.  Reducing z_i h_i modulo L changes the term by a multiple of [L]A_i, which
 * is a torsion point, and the 8 kills it (likewise for the B term, whose order is L): the verdict is a function of the batch alone, whatever the lane order
 * makes of the z_i.
 * SOUNDNESS.  Write a lane's defect [s_i]B - [h_i]A_i - R_i as its prime-order part plus a torsion part.  The lane fails rule 3 iff the prime-order part is
 * not the identity.  The prime-order part of the batch sum is then a nonzero linear form in the z_i over a group of prime order, which vanishes for at most a
 * 2^-127 fraction of the seeds (z_i is odd and takes 2^127 values), and whoever chooses the signatures does not choose the seed.
 *
 * EXECUTION.  Stream-ordered; nothing is read back; which kernels run and with how many lanes depends on (n, the message length bound, flags) ONLY: the bound
 * is msg_bytes, or stride_bytes where lens is given.  ecsimd_ed25519_batch_plan reports it.  CAPTURE, the rule of ecsimd_msm.h: the calls can be captured into
 * a graph after ONE warm-up call at the same arguments on the same context; a call that would have to grow the workspace while the stream is being captured
 * returns ECSIMD_HIP_ERR_BAD_ARG with "capture" in the message, enqueues nothing, and leaves the capture valid.
 *
 * INTERNAL CHECK, as in ecsimd_msm.h: should the sort's own invariants ever fail, ecsimd_ed25519_msm returns 32 bytes of 0xff (no encoding: y >= p),
 * finite[0] = 1 and invalid[0] = UINT32_MAX, and a batch refuses.
 *
 * ERRORS, ECSIMD_HIP_ERR_BAD_ARG with a message each: a flag that is no route (or, for the msm, asks for another route than the buckets); a null pointer;
 * lens not 4-byte aligned; stride_bytes < msg_bytes; an output overlapping an input; n above the call's bound; bits outside 1 .. 256.  The outputs are then
 * untouched.
 */
#ifndef ECSIMD_ED25519_BATCH_H
#define ECSIMD_ED25519_BATCH_H
#include "ecsimd_ed25519.h"
#include "ecsimd_msm.h"

#ifdef __cplusplus
extern "C" {
#endif

/* `flags` of ecsimd_ed25519_verify_batch and ecsimd_ed25519_batch_plan: one route, or-able with ECSIMD_ED25519_REJECT_SMALL_ORDER (bit 0).  Any other bit is
 * ECSIMD_HIP_ERR_BAD_ARG.  Both routes give the same verdict (up to the 2^-127 above). */
enum {
  ECSIMD_ED25519_BATCH_AUTO = 0,    /* LANES below ECSIMD_ED25519_BATCH_AUTO_THRESHOLD signatures, MSM from there on */
  ECSIMD_ED25519_BATCH_MSM = 2,     /* the method above */
  ECSIMD_ED25519_BATCH_LANES = 4    /* ecsimd_ed25519_verify_cofactored's kernels into a byte array of the workspace, then ONE kernel that ANDs the bytes: the
                                       same verdict with no randomizers and no 2^-127 */
};
/* Where AUTO changes route: the smallest size timed by tools/time_ed25519_batch.py from which, there and at every larger timed size, the MSM route's slowest
 * repeat is below the LANES route's fastest (one MI355X, 32-byte messages, profiles/r17/ed25519_batch.txt).
 * There MSM takes 15.1 ms against LANES' 22.1 at 2^20 signatures, 21.6 against 42.6 at 2^21, 33.9 against 85.0 at 2^22, 58.0 against 168.2 at 2^23 and 108.0
 * against 335.7 at 2^24 - 1: 155 M signatures a second, 3.11 times LANES and 2.99 times plain ecsimd_ed25519_verify (322.6 ms) in the same run.  Below that LANES
 * is faster: 6.2 ms against 13.0 at 2^18, 1.8 against 6.1 at 2^16 -- the MSM route's three dozen launches and the reduction of every bucket do not shrink with the
 * batch; 2^19 was not timed.  LANES itself costs 1.04 to 1.09 times ecsimd_ed25519_verify: the second decoding and the addition of -R. */
#define ECSIMD_ED25519_BATCH_AUTO_THRESHOLD ((size_t)1 << 20)

/* out = encode(sum over i < n of (k[i] mod 2^bits) P[i]) by the bucket method on the Edwards curve: ecsimd_msm's stages and schedule (ecsimd_msm_plan(n, bits,
 * ECSIMD_MSM_ALG_BUCKETS): c, windows, L, m, max_chain) on the complete unified addition -- about one 7-multiplication mixed addition per term and window, and
 * no branch on the group law anywhere.  k: n x 32 bytes little-endian; pts: n x 32-byte encodings; out: 32 bytes; all at any alignment.  bits in 1 .. 256.
 * Scalars are INTEGERS, not residues modulo L: the points may carry torsion and the result is the exact integer combination.  An encoding that does not decode
 * strictly is counted in invalid[0] (one uint32_t, 4-byte aligned; may be NULL) and contributes nothing.  finite[0] = 0 and the encoding of the identity
 * (01 00 .. 00) for the neutral result, n = 0 included.  flags: 0 or ECSIMD_MSM_ALG_BUCKETS -- the bucket route only.  n <= ECSIMD_MSM_MAX_N. */
int ecsimd_ed25519_msm(ecsimd_hip_ctx* ctx, const uint8_t* k, const uint8_t* pts, uint8_t* out, uint8_t* finite, uint32_t* invalid, size_t n, int bits, int flags);
/* Host only.  ecsimd_msm_plan(n, bits, ECSIMD_MSM_ALG_BUCKETS) with this call's workspace_bytes: four planes per bucket, slot and tree element where ecsimd_msm
 * has three, three planes per term where that has two beside the scalar.  launches = 8 + T(2^c / m), T as below (n = 0: 1).  Errors as ecsimd_msm_plan's. */
int ecsimd_ed25519_msm_plan(size_t n, int bits, int flags, ecsimd_msm_plan_t* out);

/* ok[i] = 1 iff lane i passes THE RULE above; one byte per lane.  flags: 0 or ECSIMD_ED25519_REJECT_SMALL_ORDER.  Any n, in chunks of 2^20 lanes.  The call
 * that names the culprits of a refused batch, and the LANES route below.  ok must not be one of the inputs. */
int ecsimd_ed25519_verify_cofactored(ecsimd_hip_ctx* ctx, const uint8_t* pk, const uint8_t* msg, size_t msg_bytes, size_t stride_bytes, const uint32_t* lens,
                                     const uint8_t* sig, uint8_t* ok, size_t n, int flags);

/* What a call will do for (n, msg_bytes, flags); msg_bytes = the message length bound (stride_bytes where lens is given).
 * launches, exact.  With T(c) = the passes of a fan-16 tree over c elements (0 for c <= 1, else 1 + T(ceil(c / 16))) and M(n, bits) =
 * ecsimd_ed25519_msm_plan(n, bits, 0).launches:
 *     n = 0:   1
 *     MSM:     5 + T(n) + max(1, T(n)) + M(n, 128) + M(n + 1, 253)
 *              (zero, front, the hash tree's T(n) levels, seed, scalars, the additions' max(1, T(n)) levels, the two sums, accept)
 *     LANES:   1 + 2 ceil(n / 2^20)
 *              (per chunk of 2^20 signatures the two kernels of ecsimd_ed25519_verify_cofactored; then the one reduction)
 * workspace_bytes: the largest need of any batch of AT MOST n signatures on that route: it never shrinks as n grows, and a context warmed up at n serves every
 * smaller batch of the same route inside a capture. */
typedef struct ecsimd_ed25519_batch_plan_t {
  int route;                 /* ECSIMD_ED25519_BATCH_MSM or ECSIMD_ED25519_BATCH_LANES: what AUTO resolves to, or the route asked for */
  int launches;
  size_t workspace_bytes;
} ecsimd_ed25519_batch_plan_t;
/* Host only: no context, no GPU.  ECSIMD_HIP_ERR_BAD_ARG for n > ECSIMD_MSM_MAX_N - 1, msg_bytes > 2^40, flags that are no route, or out == NULL. */
int ecsimd_ed25519_batch_plan(size_t n, size_t msg_bytes, int flags, ecsimd_ed25519_batch_plan_t* out);

/* ok[0] -- ONE byte -- is 1 iff every one of the n lanes passes THE RULE, with this exception on the MSM route: a batch that holds a failing lane is accepted
 * with probability at most 2^-127.  n = 0 is accepted vacuously: one kernel writes ok[0] = 1.  n <= ECSIMD_MSM_MAX_N - 1 (the B term shares the key sum); a
 * larger batch is the caller's AND over chunks.  NO LOCATING: run ecsimd_ed25519_verify_cofactored over a refused batch.  ok must not overlap an input. */
int ecsimd_ed25519_verify_batch(ecsimd_hip_ctx* ctx, const uint8_t* pk, const uint8_t* msg, size_t msg_bytes, size_t stride_bytes, const uint32_t* lens,
                                const uint8_t* sig, uint8_t* ok, size_t n, int flags);

/* z[i] = the randomizer z_i of the method above as 32 little-endian bytes (the upper 16 are 0); z: n x 32 bytes, 16-byte aligned.  The first stages of the MSM
 * route, the same kernels ecsimd_ed25519_verify_batch runs.  For tests and for a caller that wants to check the sums itself.  z must not overlap an input.
 * n = 0 does nothing; n <= ECSIMD_MSM_MAX_N - 1. */
int ecsimd_ed25519_batch_randomizers(ecsimd_hip_ctx* ctx, const uint8_t* pk, const uint8_t* msg, size_t msg_bytes, size_t stride_bytes, const uint32_t* lens,
                                     const uint8_t* sig, uint8_t* z, size_t n);

#ifdef __cplusplus
}
#endif
#endif
