/* ecsimd_schnorr_batch.h -- BIP-340 batch verification on the device: ONE verdict for a batch of Schnorr signatures on secp256k1.
 *
 * The functions live in libecsimd_hip.so beside those of ecsimd_hip.h and ecsimd_msm.h and take the same context: its stream, its grow-only workspace and its
 * error string (ecsimd_hip_last_error).  They return ECSIMD_HIP_OK or an ECSIMD_HIP_ERR_* code.  Plain C99.
 *
 * OPERANDS, as ecsimd_hip_schnorr_verify takes them: device pointers; px, r, s are n x 4 x uint64_t (little-endian limbs), 16-byte aligned; lane i's message is
 * the msg_bytes bytes at msg + i * stride_bytes (one length per call, any alignment, msg may be NULL where msg_bytes is 0).  secp256k1 only.  PUBLIC DATA ONLY:
 * the sums are ecsimd_msm's bucket method, whose memory addresses are scalar digits.
 *
 * VERDICT.  ok[0] -- ONE byte -- is 1 iff every one of the n signatures is valid under BIP-340 "Verify", with this exception: a batch that holds an invalid
 * signature is accepted with probability at most 2^-127 (below).  n = 0 is accepted vacuously: one kernel writes ok[0] = 1.  n <= ECSIMD_MSM_MAX_N - 1 (the G
 * term shares the key sum); a larger batch is the caller's AND over chunks.  NO LOCATING: a refused batch says nothing about which lane is at fault -- run
 * ecsimd_hip_schnorr_verify over it to find the culprits.
 *
 * THE METHOD (tools/schnorr_batch_model.py is the normative statement, on hashlib and big integers).  H_tag(x) = SHA256(SHA256(tag) || SHA256(tag) || x);
 * b(v) = the 32 big-endian bytes of v:
 *     E_i    = H_"BIP0340/challenge"(b(r_i) || b(px_i) || m_i), all 32 bytes;  e_i = int(E_i) mod n
 *     leaf_i = H_"ecsimd/schnorr-batch/leaf"(E_i || b(s_i))
 *     node   = H_"ecsimd/schnorr-batch/node"(c_0 || ... || c_{k-1}), k <= 16 children in lane order, level by level until one digest, the root, remains
 *     seed   = H_"ecsimd/schnorr-batch/seed"(root || n as 8 big-endian bytes);  n = 1: the root is leaf_0
 *     a_i    = (int(H_"ecsimd/schnorr-batch/a"(seed || i as 8 big-endian bytes)) mod 2^128) | 1
 * and, with P_i and R_i the even-y points of x = px_i and x = r_i, the batch is accepted iff every lane is well formed (both points exist, s_i < n) and
 *     sum a_i R_i  +  [ sum (a_i e_i mod n) P_i + (n - sum a_i s_i mod n) G ]  =  the point at infinity.
 * The seed is a hash of every input, which is BIP-340's own recommendation: the caller supplies no entropy and cannot get the randomizers wrong, and the call
 * is deterministic -- the same batch gives the same a_i, in a test and in a replayed graph.  Every a_i is odd, hence nonzero without a branch, and takes 2^127
 * values; every lane has one, lane 0 included.  SOUNDNESS: where some lane is not a valid signature the left side is a nonzero linear form in the a_i over a
 * group of prime order, so it vanishes for at most a 2^-127 fraction of the seeds, and whoever chooses the signatures does not choose the seed.
 *
 * EXECUTION.  Stream-ordered; nothing is read back; which kernels run and with how many lanes depends on (n, msg_bytes, flags) ONLY.  ecsimd_schnorr_batch_plan
 * reports it.  CAPTURE, the rule of ecsimd_msm.h: the calls can be captured into a graph after ONE warm-up call at the same (n, msg_bytes, flags) on the same
 * context; a call that would have to grow the workspace (or build a table) while the stream is being captured returns ECSIMD_HIP_ERR_BAD_ARG with "capture" in
 * the message, enqueues nothing, and leaves the capture valid.
 *
 * ERRORS, ECSIMD_HIP_ERR_BAD_ARG with a message each: a context with ECSIMD_HIP_REF_SQUARE_COMPAT set (as ecsimd_hip_schnorr_verify refuses it); a flag that
 * is no route; a null or misaligned pointer; ok or a overlapping an input; n above ECSIMD_MSM_MAX_N - 1.  ok[0] is then untouched.
 */
#ifndef ECSIMD_SCHNORR_BATCH_H
#define ECSIMD_SCHNORR_BATCH_H
#include "ecsimd_msm.h"

#ifdef __cplusplus
extern "C" {
#endif

/* `flags` of ecsimd_schnorr_verify_batch: the route.  Any other bit is ECSIMD_HIP_ERR_BAD_ARG.  Both routes give the same verdict (up to the 2^-127 above). */
enum {
  ECSIMD_SCHNORR_BATCH_AUTO = 0,   /* LANES below ECSIMD_SCHNORR_BATCH_AUTO_THRESHOLD signatures, MSM from there on */
  ECSIMD_SCHNORR_BATCH_MSM = 1,    /* the method above: two bucket sums (ECSIMD_MSM_ALG_BUCKETS; 128-bit scalars over n terms, 256-bit scalars over n + 1) */
  ECSIMD_SCHNORR_BATCH_LANES = 2   /* ecsimd_hip_schnorr_verify's own path into a byte array of the workspace, then ONE kernel that ANDs the bytes: the same
                                      verdict with no randomizers and no 2^-127.  The route for small n */
};
/* Where AUTO changes route: the smallest size timed by tools/time_schnorr_batch.py from which, there and at every larger timed size, the MSM route's slowest
 * repeat is below the LANES route's fastest (one MI355X, 32-byte messages, profiles/r16/schnorr_batch.txt).  There MSM takes 35.1 ms against LANES' 42.8 at
 * 2^22 signatures, 60.4 against 82.5 at 2^23 and 109.7 against 163.3 at 2^24 - 1; at 2^21 the two are inside each other's repeat spread (22.9 against 22.6 ms)
 * and below that LANES is faster: 11.9 ms against 16.5 at 2^20, 1.0 against 6.1 at 2^16 -- the MSM route's three dozen launches, its second square root per
 * signature and the reduction of every bucket do not shrink with the batch.  LANES itself costs 1.01 to 1.10 times plain ecsimd_hip_schnorr_verify in that run. */
#define ECSIMD_SCHNORR_BATCH_AUTO_THRESHOLD ((size_t)1 << 22)

/* What a call will do for (n, msg_bytes, flags).
 * launches, exact.  With T(c) = the passes of a fan-16 tree over c elements (0 for c <= 1, else 1 + T(ceil(c / 16))) and M(n, bits) = ecsimd_msm_plan(n, bits,
 * ECSIMD_MSM_ALG_BUCKETS).launches:
 *     n = 0:   1
 *     MSM:     5 + T(n) + max(1, T(n)) + M(n, 128) + M(n + 1, 256)
 *              (zero, front, the hash tree's T(n) levels, seed, scalars, the additions' max(1, T(n)) levels, the two sums, accept)
 *     LANES:   1 + 9 ceil(n / 2^22)
 *              (per chunk of 2^22 signatures ecsimd_hip_schnorr_verify's nine kernels: its front, s G, that product's inversion, the three of e P, the
 *              addition, the clearing of invalid lanes, its accept; then the one reduction)
 * workspace_bytes: the context workspace the call asks for: the largest need of any batch of AT MOST n signatures on that route, so it never shrinks as n grows
 * and a context warmed up at n serves every smaller batch of the same route inside a capture.  (The bucket sums' own need is not monotone in the number of terms.) */
typedef struct ecsimd_schnorr_batch_plan_t {
  int route;                 /* ECSIMD_SCHNORR_BATCH_MSM or ECSIMD_SCHNORR_BATCH_LANES: what AUTO resolves to, or the route asked for */
  int launches;
  size_t workspace_bytes;
} ecsimd_schnorr_batch_plan_t;
/* Host only: no context, no GPU.  ECSIMD_HIP_ERR_BAD_ARG for n > ECSIMD_MSM_MAX_N - 1, msg_bytes > 2^40, a flag that is no route, or out == NULL. */
int ecsimd_schnorr_batch_plan(size_t n, size_t msg_bytes, int flags, ecsimd_schnorr_batch_plan_t* out);

/* ok[0] = the verdict for the whole batch.  ok must not overlap an input. */
int ecsimd_schnorr_verify_batch(ecsimd_hip_ctx* ctx, const uint64_t* px, const uint8_t* msg, size_t msg_bytes, size_t stride_bytes,
                                const uint64_t* r, const uint64_t* s, uint8_t* ok, size_t n, int flags);

/* a[i] = the randomizer a_i of the method above (n x 4 words, 16-byte aligned, the upper two words 0): the first three stages of the MSM route, the same kernels
 * ecsimd_schnorr_verify_batch runs.  For tests and for a caller that wants to check the sums itself.  a must not overlap an input.  n = 0 does nothing. */
int ecsimd_schnorr_batch_randomizers(ecsimd_hip_ctx* ctx, const uint64_t* px, const uint8_t* msg, size_t msg_bytes, size_t stride_bytes,
                                     const uint64_t* r, const uint64_t* s, uint64_t* a, size_t n);

#ifdef __cplusplus
}
#endif
#endif
