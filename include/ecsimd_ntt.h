/* ecsimd_ntt.h -- the number-theoretic transform on the device, over BLS12-381's scalar field Fr or any prime field registered with
 * ecsimd_hip_register_modulus(.., ECSIMD_HIP_MODULUS_PRIME, ..): evaluations <-> coefficients on a subgroup of roots of unity or a coset of it, the bit-reversal
 * permutation, and (with ecsimd_hip_mod_mul) polynomial products.  The other half of a KZG / PLONK prover beside the multi-scalar multiplications.
 *
 * The functions live in libecsimd_hip.so beside those of ecsimd_hip.h and take the same context: its stream, its grow-only workspace and its error string
 * (ecsimd_hip_last_error).  They return ECSIMD_HIP_OK or a negative ECSIMD_HIP_ERR_* code.  Plain C99.
 *
 * ELEMENTS are those of ecsimd_hip.h: 4 x uint64_t, little-endian limbs, 32 bytes, one after the other -- also the scalar format of ecsimd_msm and of the
 * BLS12-381 sums, so a transform's output feeds them unconverted.  Every array pointer is a device pointer, 16-byte aligned.  Inputs are ANY 256-bit values, taken
 * modulo p; outputs are canonical (below p) and classical (no Montgomery form crosses this interface).
 *
 * DOMAIN.  p - 1 = 2^s m, m odd: s is the field's two-adicity.  A domain of size n = 2^log_n is H = {w^k}, w = root^(2^(s - log_n)) for a primitive 2^s-th root
 * of unity `root`, or a coset g H of it.  The DEFAULT root of a field is g0^((p - 1) / 2^s) for the smallest integer g0 >= 2 that is a quadratic non-residue
 * (ecsimd_ntt_field_info).  For Fr the ecosystem's root is 7^((r - 1) / 2^32) -- NOT the default rule's, since 5 is Fr's smallest non-residue --:
 * ecsimd_ntt_bls12_381_fr returns that one, and a caller who wants it passes it to ecsimd_ntt_domain_create.
 *
 * PUBLIC OR SECRET-INDEPENDENT.  Nothing here is constant-time in the strict sense or wiped, but a transform's memory addresses and branches depend only on
 * (log_n, batch, flags), never on the values: the butterflies are the field layer's add / subtract / Montgomery product, which select and do not branch.
 *
 * SCHEDULE.  A transform is `passes` kernel launches, each over the whole batch; ecsimd_ntt_plan reports them.  Stream-ordered, nothing is read back.
 * CAPTURE: the transforms and ecsimd_ntt_bitrev only enqueue kernels on the context's stream.  With workspace_bytes = 0 (one pass: n <= 2^9 at the default
 * schedule) a call can be captured into a graph without a warm-up.  Otherwise it follows ecsimd_msm's rule: ONE warm-up call at the same (log_n, batch, flags) on
 * the same context grows the workspace; a call that would have to grow it while the stream is being captured returns ECSIMD_HIP_ERR_BAD_ARG with "capture" in
 * the message, enqueues nothing, and leaves the capture valid.  ecsimd_ntt_domain_create and _destroy allocate and wait: they refuse inside a capture.
 */
#ifndef ECSIMD_NTT_H
#define ECSIMD_NTT_H
#include "ecsimd_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ECSIMD_NTT_MAX_LOG_N 24              /* 2^24 elements per transform: ecsimd_msm's cap too */
#define ECSIMD_NTT_MAX_PASSES 24
#define ECSIMD_NTT_DEFAULT_RADIX_LOG 9       /* a pass runs at most 9 butterfly stages: 2^9 rows x 4 columns fill a workgroup's 2^11-element tile */
/* `flags` of the transforms and of ecsimd_ntt_plan: 0, or ECSIMD_NTT_MAX_RADIX_LOG(r) with 1 <= r <= ECSIMD_NTT_DEFAULT_RADIX_LOG, which caps every pass's
 * log-radix at r.  It is a TEST HOOK: it reaches the multi-pass code at 2^2 elements instead of 2^10 (three passes at 2^3 instead of 2^19), computes the same
 * values, and is slower -- more passes over memory.  Any other bit is ECSIMD_HIP_ERR_BAD_ARG. */
#define ECSIMD_NTT_MAX_RADIX_LOG(r) ((r) & 15)

/* What a transform of `batch` arrays of 2^log_n elements will do: a function of (log_n, batch, flags) alone.  The stages are spread evenly over the fewest passes
 * the cap allows, the wider passes first: log_n = 19 runs 7 + 6 + 6.  Every pass reads and writes each element once. */
typedef struct ecsimd_ntt_plan_t {
  int passes;                                /* kernel launches of one transform call */
  int log_radix[ECSIMD_NTT_MAX_PASSES];      /* butterfly stages of pass i; 0 behind the last pass */
  int lanes;                                 /* per workgroup */
  int lds_bytes;                             /* per workgroup: two planes of 16-byte half elements, rows padded by one slot */
  int launches;                              /* = passes */
  size_t workspace_bytes;                    /* 0 for one pass; else batch * 2^log_n * 32: the buffer the passes alternate with `out` */
} ecsimd_ntt_plan_t;
/* Host only: no context, no GPU.  ECSIMD_HIP_ERR_BAD_ARG for log_n outside 1 .. 24, batch = 0 or batch * 2^log_n > 2^38, a bad flag, or out == NULL. */
int ecsimd_ntt_plan(int log_n, size_t batch, int flags, ecsimd_ntt_plan_t* out);

/* Host only.  field: a field id -- a modulus registered as PRIME, a registered curve's id (its prime), ECSIMD_HIP_P256 / ECSIMD_HIP_SECP256K1 (the curve primes)
 * or ECSIMD_HIP_FIELD_*_ORDER (the group orders).  A modulus registered without ECSIMD_HIP_MODULUS_PRIME is refused.  two_adicity = s; root = the default root,
 * classical.  Either output may be NULL. */
int ecsimd_ntt_field_info(int field, int* two_adicity, uint64_t root[4]);

/* Host only.  Registers r = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001 as a prime modulus, returns its field id and the CONVENTIONAL
 * root 7^((r - 1) / 2^32) = 0x16a2a19edfe81f20d09b681922c813b4b63683508c2280b93829971f439f0d2b -- not ecsimd_ntt_field_info's, which starts from 5. */
int ecsimd_ntt_bls12_381_fr(int* field, uint64_t root[4]);

/* A domain: the device tables of one (field, log_n, root, shift) -- the powers of w and of 1/w, of g and of 1/g in two levels (x^i = lo[i mod 2^12] hi[i div 2^12]:
 * 2^12 + 2^(log_n - 12) entries instead of 2^log_n), and 1/n, all in Montgomery form.  It belongs to the context that made it.
 *   1 <= log_n <= min(s, 24).  root: a primitive 2^s-th root of unity (refused unless root < p and root^(2^(s-1)) = -1), or NULL for the default.
 *   shift: NULL or 1 for the subgroup H; any other 0 < g < p for the coset g H; 0 or >= p is refused.
 * Builds the tables, uploads them and synchronises the context's stream.  Destroy it before the context, outside any capture. */
typedef struct ecsimd_ntt_domain ecsimd_ntt_domain;
int ecsimd_ntt_domain_create(ecsimd_hip_ctx* ctx, int field, int log_n, const uint64_t root[4], const uint64_t shift[4], ecsimd_ntt_domain** dom);
int ecsimd_ntt_domain_destroy(ecsimd_hip_ctx* ctx, ecsimd_ntt_domain* dom);

/* For each of `batch` consecutive arrays of n elements: out[k] = sum over i of in[i] (g w^k)^i mod p.  Natural order in and out.  out == in is allowed; any other
 * overlap of the two is refused.  batch = 0 succeeds. */
int ecsimd_ntt_forward(ecsimd_hip_ctx* ctx, const ecsimd_ntt_domain* dom, const uint64_t* in, uint64_t* out, size_t batch, int flags);
/* The exact inverse, 1/n and g^-i included: ecsimd_ntt_inverse(ecsimd_ntt_forward(x)) = x mod p on any domain. */
int ecsimd_ntt_inverse(ecsimd_hip_ctx* ctx, const ecsimd_ntt_domain* dom, const uint64_t* in, uint64_t* out, size_t batch, int flags);

/* The bit-reversal permutation of each array: out[rev(i)] = in[i], rev = the log_n-bit reversal.  1 <= log_n <= 24; out == in is allowed, any other overlap is
 * refused.  It takes no field: the elements are moved, not read.  (EIP-4844 and several provers keep evaluation form in this order; there are no fused
 * bit-reversed transform modes -- the permutation is one pass over memory.)  One launch, no workspace. */
int ecsimd_ntt_bitrev(ecsimd_hip_ctx* ctx, int log_n, const uint64_t* in, uint64_t* out, size_t batch);

#ifdef __cplusplus
}
#endif
#endif
