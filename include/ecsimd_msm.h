/* ecsimd_msm.h -- multi-scalar multiplication on the device: R = sum k_i P_i over a batch by the bucket method (Pippenger), and the sum of a batch of points.
 *
 * The functions live in libecsimd_hip.so beside those of ecsimd_hip.h and take the same context: its stream, its grow-only workspace and its error string
 * (ecsimd_hip_last_error).  They return ECSIMD_HIP_OK or an ECSIMD_HIP_ERR_* code.  Plain C99.
 *
 * Every other entry point of the library is lane-parallel -- one scalar, one point, one result per lane.  These two sum ACROSS lanes: the result is ONE point.
 *
 * Common to both calls: every pointer is a device pointer, 16-byte aligned; k, x, y are n x 4 x uint64_t in the layout of ecsimd_hip.h (little-endian limbs),
 * points affine classical, (0, 0) the point at infinity, which contributes nothing.  The result is rx, ry (4 words each, affine classical, (0, 0) at
 * infinity) and finite[0] (1 or 0).  n = 0 succeeds: the empty sum is infinity, (0, 0) with finite = 0.  Every input point is VALIDATED as ecsimd_hip_on_curve
 * validates (both coordinates below p, on the curve): an invalid point is treated as infinity and counted in invalid[0] (one uint32_t; may be NULL).  Curves:
 * ECSIMD_HIP_P256 and ECSIMD_HIP_SECP256K1; a curve registered at run time is refused (ECSIMD_HIP_ERR_BAD_ARG, "registered curves have no multi-scalar
 * multiplication").  No ECSIMD_HIP_REF_SQUARE_COMPAT form: a context with that option set is accepted and computes the same bytes (only the affine sum is
 * promised, and the inverse of a field element is unique).
 *
 * PUBLIC DATA ONLY.  Both calls are table-driven algorithms whose memory addresses are scalar digits, and every exceptional case of the group law is a branch:
 * for PUBLIC scalars and points only -- the words ecsimd_hip.h uses for its ALG_* flags apply to every route here, ECSIMD_MSM_ALG_LANES included
 * (it runs ECSIMD_HIP_ALG_WINDOWED).
 *
 * SCHEDULE.  Which kernels run, with how many lanes and how long a lane's loop is, depends on (n, bits, flags) ONLY, never on the data; nothing is read back.
 * ecsimd_msm_plan reports it.  Stream-ordered.  CAPTURE: the calls only enqueue kernels and can be captured into a graph after ONE warm-up call at the same
 * (n, bits, flags) on the same context -- the warm-up grows the workspace (ecsimd_msm_plan's workspace_bytes); a call that would have to grow it while the
 * stream is being captured returns ECSIMD_HIP_ERR_BAD_ARG with "capture" in the message, enqueues nothing, and leaves the capture valid.
 *
 * INTERNAL CHECK.  The bucket route's sort checks its own invariants on the device (every sorted entry names a term, every bucket's offsets are a scan of the
 * histogram).  Should one ever fail, the call does not return a sum that only looks right: rx and ry are 32 bytes of 0xff (no field element), finite[0] = 1
 * and invalid[0] = UINT32_MAX.  A batch verification that accepts on finite[0] == 0 therefore refuses.
 */
#ifndef ECSIMD_MSM_H
#define ECSIMD_MSM_H
#include "ecsimd_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ECSIMD_MSM_MAX_N ((size_t)1 << 24)   /* terms per ecsimd_msm call; a longer sum is chunks chained through ecsimd_msm_point_sum */

/* `flags` of ecsimd_msm: the route.  Any other bit is ECSIMD_HIP_ERR_BAD_ARG.  All routes give the same affine bytes. */
enum {
  ECSIMD_MSM_ALG_AUTO = 0,     /* LANES below ECSIMD_MSM_AUTO_THRESHOLD terms, BUCKETS from there on */
  ECSIMD_MSM_ALG_BUCKETS = 1,  /* the bucket method: c-bit unsigned digits (digit 0 skipped), a counting sort by (window, digit), segmented bucket sums with
                                  complete mixed additions -- roughly ONE mixed addition (11 field multiplications) per term and window --, the running-sum
                                  bucket reduction in chunks, c doublings per window, one inversion.  NOT for secret scalars: bucket addresses are scalar digits */
  ECSIMD_MSM_ALG_LANES = 2     /* per-lane k_i P_i by ecsimd_hip_scalar_mult's ECSIMD_HIP_ALG_WINDOWED (about 2 770 field multiplications per term), then the
                                  tree sum of ecsimd_msm_point_sum: the route for small n and the on-device cross-check of the other.  NOT for secret scalars */
};
/* Where AUTO changes route: the measured crossover at bits = 256, rounded up to a power of two (tools/time_msm.py, one MI355X, profiles/r15/msm.txt).  There
 * BUCKETS takes 6.2 ms against LANES' 4.6 (P-256) / 3.1 (secp256k1) at 2^18 terms and 7.7 / 7.8 ms against 15.4 / 10.2 at 2^20; 2^19 was not timed.  With
 * bits = 128 BUCKETS is already faster at 2^18 (2.6 ms against 4.5 / 3.0): a caller with short scalars and 2^18 terms or more asks for BUCKETS itself.  Below
 * the crossover BUCKETS' dozen launches, its reduction of every one of 2^c buckets and the lanes its slices leave idle cost more than the per-lane products. */
#define ECSIMD_MSM_AUTO_THRESHOLD ((size_t)1 << 20)

/* What a call will do for (n, bits, flags).  A field that does not apply to the route is 0.
 * THE SERIAL BOUND.  No lane of any kernel executes more than max_chain point operations (additions or doublings) one after the other, whatever the scalars:
 *     max_chain = max(L, ceil(n / L) + 1, 2 m + 2 c, 16, windows (c + 1))        (BUCKETS)
 * with L = max(4, 2^ceil(ceil(log2 n) / 2) / 4) <= 2 sqrt(n): the segment split.  A run of equal digits longer than L is cut into slices summed by different lanes
 * (at most L mixed additions each) and the slices' sums are combined by the bucket's lane (at most ceil(n / L) + 1 additions: a bucket has at most n entries).
 * So a batch in which every scalar is the same costs one lane O(sqrt n) additions, not n.  2 m + 2 c is a lane of the bucket reduction, 16 the tree sum's
 * fan-in, windows (c + 1) < bits + c + windows the last lane's doublings and additions (no function of n).  tools/msm_model.py emulates the stages index by index and counts. */
typedef struct ecsimd_msm_plan_t {
  int route;                 /* ECSIMD_MSM_ALG_BUCKETS or ECSIMD_MSM_ALG_LANES: what AUTO resolves to, or the route asked for */
  int c;                     /* BUCKETS: the window width in bits: ceil(bits / windows), windows being what c0 = min(bits, min(16, max(2, floor(log2 n) - 4))) needs */
  int windows;               /* BUCKETS: ceil(bits / c0) = ceil(bits / c): evenly wide windows, no narrow top one */
  uint32_t buckets;          /* BUCKETS: 2^c per window, bucket 0 never summed */
  uint32_t L;                /* BUCKETS: the segment split length, in entries of the sorted array */
  uint32_t m;                /* BUCKETS: buckets per lane of the bucket reduction: min(2^c, max(2, min(32, 2^ceil(c / 2)))) */
  uint32_t max_chain;        /* the serial bound above (LANES: the tree sum's fan-in; the per-lane product is ecsimd_hip_scalar_mult's own) */
  int launches;              /* kernels enqueued.  BUCKETS: exact.  LANES: an UPPER BOUND -- the per-lane product counts as five kernels per 2^22 terms,
                                which is P-256's number; secp256k1's takes three */
  size_t workspace_bytes;    /* context workspace the call needs */
} ecsimd_msm_plan_t;
/* Host only: no context, no GPU.  ECSIMD_HIP_ERR_BAD_ARG for bits outside 1 .. 256, n > ECSIMD_MSM_MAX_N, a flag bit that is no route, or out == NULL. */
int ecsimd_msm_plan(size_t n, int bits, int flags, ecsimd_msm_plan_t* out);

/* R = sum over i < n of (k[i] mod 2^bits) P[i].  bits in 1 .. 256: ONLY the low `bits` bits of each scalar are read, so a caller with 128-bit randomizers pays
 * for half the windows (the upper words may hold anything).  n <= ECSIMD_MSM_MAX_N.  An output must not be one of the inputs or another output. */
int ecsimd_msm(ecsimd_hip_ctx* ctx, int curve, const uint64_t* k, const uint64_t* x, const uint64_t* y,
               uint64_t* rx, uint64_t* ry, uint8_t* finite, uint32_t* invalid, size_t n, int bits, int flags);

/* R = sum over i < n of P[i]: the tree sum behind a validating front -- lanes own strided slices of 16 points, one launch per level, complete additions.
 * Any n; ecsimd_msm_plan(n', 1, ECSIMD_MSM_ALG_LANES) does not describe it: its workspace is 96 bytes per 16 points and its launches 2 + max(1, ceil(log16 n)). */
int ecsimd_msm_point_sum(ecsimd_hip_ctx* ctx, int curve, const uint64_t* x, const uint64_t* y,
                         uint64_t* rx, uint64_t* ry, uint8_t* finite, uint32_t* invalid, size_t n);

#ifdef __cplusplus
}
#endif
#endif
