/*
 * ecsimd_hip.h -- C ABI of the MI355X (gfx950) batched elliptic-curve engine.
 *
 * This is the drop-in boundary for the hot path of aguinet/ecsimd.  The
 * reference is header-only C++ with no ABI of its own: its single linkable symbol is
 * scalar_mult_p256 (lib/scalar_mult_p256.cpp:10-12).  Every entry point below replaces one
 * reference function (cited per declaration) over a RUNTIME-LENGTH batch; n = 4 reproduces one
 * eve::wide of the reference.  The C++ headers in include/ecsimd/ bind these symbols and keep
 * the reference's names (curve_group<Curve>::scalar_mult, DBLU, ZADDU, ZDAU, ADD_Z2_1,
 * scalar_mult_p256, ...).  INTEGRATION.md shows the binding a maintainer of the reference adds.
 *
 * Data layout (all pointers are DEVICE pointers, 16-byte aligned):
 *   field element / scalar : 4 x uint64_t, little-endian limb order (limb 0 least significant),
 *                            = the reference's bignum<uint64_t,4> (bignum.h:38-99,
 *                            serialization.h:18-21).  A batch is AoS: element i at p + 4*i.
 *   512-bit product        : 8 x uint64_t per element.
 *   point batch            : one array per coordinate (x[], y[], z[]).  Jacobian coordinates are
 *                            in Montgomery form (jacobian_curve_point.h:25-31), affine ones are
 *                            classical unless the function name says _mgry.
 *   flags                  : one uint8_t per element (0/1).
 * Preconditions the reference only asserts in debug builds (co-Z inputs, Z = mgry(1) for
 * DBLU / ADD_Z2_1 / scalar_mult) are the caller's responsibility here too.
 *
 * Every call enqueues kernels on the context's stream and returns without synchronising;
 * ecsimd_hip_sync() waits.  Return value: 0 on success, negative ecsimd_hip_status otherwise.
 * Nothing throws across this boundary.  A context is not thread-safe: one per host thread/GPU.
 */
#ifndef ECSIMD_HIP_H
#define ECSIMD_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ecsimd_hip_ctx ecsimd_hip_ctx;

enum ecsimd_hip_curve {
  ECSIMD_HIP_P256 = 0,      /* curve_nist_p256.h:14-32 */
  ECSIMD_HIP_SECP256K1 = 1, /* prime of tests/mgry.cpp:25-27 with a=0, b=7 (SEC 2) */
  ECSIMD_HIP_FIRST_REGISTERED_CURVE = 0x10000  /* ids of ecsimd_hip_register_curve start here (r5): curve_group<Curve> for ANY Curve type, curve.h:12-15 */
};

/* FIELD ids: what the element-wise field entry points (mod_*, mgry_*, gfp_*, get_constant) take as `curve`.  The reference's field layer is
 * generic in the modulus type P (mgry_mul.h:84-121 details::mgry_reduce<P>, mgry_csts.h:15-35 mgry_constants<WBN, P>, gfp.h:17-115 GFp<WBN, P>);
 * here a modulus is a run-time value with an id.  0, 1: the curve primes above (hand-laid special-form kernels); 2, 3: the two group orders n
 * (what ECDSA computes modulo); 4...: moduli registered with ecsimd_hip_register_modulus; a curve id of ecsimd_hip_register_curve names its prime's field. */
enum ecsimd_hip_field {
  ECSIMD_HIP_FIELD_P256_ORDER = 2,      /* n of P-256 (SP 800-186 3.2.1.3) */
  ECSIMD_HIP_FIELD_SECP256K1_ORDER = 3  /* n of secp256k1 (SEC 2 v2 2.4.1) */
};
enum { ECSIMD_HIP_MODULUS_PRIME = 1 };  /* register_modulus: the caller vouches that p is PRIME; gfp_inverse then uses the constant-time division-step
                                           inversion with one shared inversion per up to 128 elements (the unique inverse = x^(p-2)).  Without it
                                           gfp_inverse raises to p - 2 bit by bit -- gfp.h:42-44 as written, the reference's value for ANY odd p */

enum ecsimd_hip_status {
  ECSIMD_HIP_OK = 0,
  ECSIMD_HIP_ERR_BAD_ARG = -1,     /* null pointer, unknown curve, misaligned pointer */
  ECSIMD_HIP_ERR_NO_DEVICE = -2,   /* no HIP device / wrong architecture (gfx950 code object only) */
  ECSIMD_HIP_ERR_HIP = -3          /* a HIP runtime call failed; see ecsimd_hip_last_error() */
};

/* scalar_mult flags.  SECRET SCALARS: only the default algorithm (no ALG_* bit: the reference's co-Z ladder, and its Z-less
 * form for x-only P-256 output) is constant-time -- one instruction stream, no branch or address that depends on a scalar
 * bit or an intermediate value, checked on the shipped ISA by tests/test_constant_time_isa.py.  Every ALG_* bit selects a
 * table-driven algorithm whose memory addresses are scalar digits: for PUBLIC scalars only (each flag says so below). */
enum {
  ECSIMD_HIP_BASE_CLASSICAL = 0,   /* base point (x, y) classical: from_affine is applied first */
  ECSIMD_HIP_BASE_MGRY = 1,        /* base point already Montgomery form (what scalar_mult_p256 receives) */
  ECSIMD_HIP_BASE_GENERATOR = 512, /* ecsimd_hip_scalar_mult only, with x = y = NULL: the base point is the curve generator (= ecsimd_hip_scalar_mult_base).
                                      Two null pointers WITHOUT this flag are ECSIMD_HIP_ERR_BAD_ARG, like any other null pointer */
  ECSIMD_HIP_OUT_JACOBIAN = 0,     /* out = (X, Y, Z) Montgomery form, as curve_group::scalar_mult returns */
  ECSIMD_HIP_OUT_AFFINE = 2,       /* out = to_affine(): (x, y) classical; oz may be NULL; oy may be NULL too: the x coordinate only
                                      (ECDH's shared secret, ECDSA's r): the conversion then skips y's two field multiplications, and on P-256 the
                                      ladder itself (no ALG_* flag, no REF_SQUARE_COMPAT) runs WITHOUT the Z coordinate -- 8M + 6S per bit instead
                                      of 9M + 7S, x recovered from the two co-Z results and the curve equation, 55 M/s against 48 -- on the odd one
                                      of k mod n and n - k mod n.  Same constant-time shape as the ladder; correct for EVERY 256-bit k (x = 0 for
                                      k = 0 mod n), including the reference ladder's degenerate scalars */
  ECSIMD_HIP_ALG_WINDOWED = 4,     /* with OUT_AFFINE only.  scalar_mult_base: 4-bit windows over an LDS-resident table (32 KiB: the odd
                                      multiples (2d+1)*16^w*G; the odd one of k mod n, n - k is recoded into 64 odd digits, so the sum is
                                      63 mixed additions with no zero digit to skip) and one simultaneous inversion instead of the
                                      reference's ladder.
                                      scalar_mult / double_scalar_mult (variable base): a per-element table of 8 multiples
                                      of P in device memory and signed 4-bit windows (odd digits, 3 doublings + one fused
                                      double-add per window: ~2 770 field multiplications against the ladder's 4 064;
                                      secp256k1 splits k = k1 + k2*lambda first), 1 408 B of context workspace per
                                      element, at most 2^22 elements at a time.  Same affine result as
                                      the ladder for every k except the ladder's degenerate scalars k = n-1, 2^256-n-1,
                                      2^256-n (there the reference returns a meaningless point, these paths the right
                                      one); k = 0 mod n -> (0, 0).  NOT for secret scalars: table reads (LDS for the fixed
                                      base, device memory for the per-element tables) are indexed by scalar digits --
                                      unless ALG_CONSTANT_TIME is added (below) */
  ECSIMD_HIP_ALG_WINDOWED_SIGNED = 8, /* as ALG_WINDOWED with signed 7-bit windows: 36 mixed additions instead of 63, a 148 KiB
                                      table of the odd multiples (2d+1)*2^(7i)*G (d = 0..63) in LDS, negative digits negate y; same results.
                                      NOT for secret scalars (LDS reads indexed by scalar digits) */
  ECSIMD_HIP_ALG_NO_ENDOMORPHISM = 16, /* secp256k1 + ALG_WINDOWED on a variable base splits k = k1 + k2*lambda (GLV) and runs
                                      half as many windows; this flag keeps the plain odd-digit loop of 63 windows (same results);
                                      a modifier of ALG_WINDOWED: NOT for secret scalars either way */
  ECSIMD_HIP_REF_SQUARE_COMPAT = 64, /* ladder only: square with the reference's square() AS WRITTEN (mul.h:160-212), which drops a
                                      carry at mul.h:186-190 (its "TODO: carry?", mul.h:207) on ~2e-9 of random operands -- ~3e-6 of
                                      random scalar multiplications then differ from the exact result.  With this flag (or the
                                      context option below) the output is the reference's bits on EVERY input, at ~0.9x the speed;
                                      without it, it is the exact k*P (what the reference's own tests assume).  Same ladder, same
                                      constant-time shape: safe for secret scalars */
  ECSIMD_HIP_ALG_CONSTANT_TIME = 128, /* a modifier of ALG_WINDOWED (r3): the table-driven algorithms WITHOUT a scalar-dependent address or branch -- every
                                      lane reads ALL entries a window could pick and keeps its own under lane masks; the recodings have no zero digit,
                                      exceptional scalars and k = 0 mod n are handled by selects (tools/ct_check.py checks the shipped ISA of the window
                                      loops, tests/test_constant_time_isa.py).  SAFE for secret scalars; same results as ALG_WINDOWED.
                                      scalar_mult_base: an odd-digit comb over an LDS table -- one address per wave, an LDS broadcast (52 five-bit
                                      windows x 16 entries, 51 additions, three 256-thread workgroups per CU): k*G for key generation and ECDSA
                                      nonces at 6.3x the ladder's rate (P-256 368 M/s, secp256k1 365 M/s).
                                      scalar_mult / scalar_mult_1s: the per-element window tables with all 8 entries of the lane's own table (512
                                      contiguous bytes) read in every window; on secp256k1 the GLV split stays, run on the COMPLETE addition law of
                                      a = 0 curves (no exceptional case to branch on; ALG_NO_ENDOMORPHISM: the plain odd-digit loop).  ECDH with a
                                      secret scalar at 1.33x (P-256: 78.2 M/s) / 1.67x (secp256k1: 99.8 M/s) the round-4 ladder's rate
                                      (oy = NULL works here too).  Not with ALG_WINDOWED_SIGNED / ALG_WINDOWED_BIG (64 or 2^19 entries per window to read).
                                      Without ALG_WINDOWED the flag is refused by every entry point (the ladder is constant-time as it is);
                                      double_scalar_mult / ecdsa_verify* take no flags: they are for public data */
  ECSIMD_HIP_LADDER_RADIX32 = 256, /* ladder only (r4): run the 254 iterations on 8 x 32-bit canonical words (the kernel of rounds 1-3) instead of the
                                      reduced-radix loop (nine signed 29-bit limbs, carry-free columns: fe29.cuh) that is the default since round 4.
                                      The field values of every iteration are the same, so X, Y, Z are bit-identical; kept for A/B measurements.
                                      REF_SQUARE_COMPAT implies it (the dropped carry depends on the 32-bit Montgomery digits).  Same constant-time shape */
  ECSIMD_HIP_ALG_WINDOWED_BIG = 32 /* scalar_mult_base + OUT_AFFINE: 20-bit windows with odd digits over a 436 MB table of the odd
                                      multiples (2d+1)*2^(20i)*G (13 windows x 2^19 entries) in device memory, built on first
                                      use (0.23 s per curve): 12 mixed additions per scalar; same results.  NOT for secret scalars:
                                      each window is a 64-byte read from device memory at an address formed from 20 scalar bits */
};

/* ---- context, stream and memory ------------------------------------------------------- */
int ecsimd_hip_init(int device, ecsimd_hip_ctx** ctx);
/* Waits for the context's stream, then frees everything the context owns.  Not while that stream is being captured (see STREAM CAPTURE below). */
int ecsimd_hip_destroy(ecsimd_hip_ctx* ctx);
/* Run on a caller-owned hipStream_t (e.g. torch's current stream).  NULL is HIP's default (null)
 * stream -- which is what torch's default stream is -- not "none".  The context's scratch memory is ordered
 * by its stream: switching makes the new stream wait (by event, no host synchronisation) for the work this
 * context enqueued on the previous one, which must still exist at that moment.  Streams under hipGraph capture are
 * selected without that hand-off (the caller brackets the capture: synchronise, capture, synchronise).
 *
 * STREAM CAPTURE.  Every entry point is in one of three classes (tests/capture_matrix.py holds the list to this header):
 *   - it only ENQUEUES on the context's stream -- kernel launches, the hipMemsetAsync wipes of secret workspace, device-to-device copies -- and is
 *     capturable once its first call at the capture's batch size has sized the context workspace and built the tables it uses (those steps allocate and
 *     synchronise).  Every compute entry point not listed below is of this kind, and so are set_stream, use_own_stream and memcpy_d2d.  Host scalars and
 *     the few-word host arrays (mgry_pow's exponent, scalar_mult_1s's k1) are kernel arguments: a graph replays the values it was captured with.  The
 *     wipes are nodes of the graph: a replay leaves the workspace as clean as the eager call does.  A call that would have to grow the workspace or build a
 *     table WHILE its stream is being captured returns ECSIMD_HIP_ERR_BAD_ARG instead (growing frees the old block, which an earlier capture may still
 *     point into): warm up at the largest batch size, then capture;
 *   - it NEEDS THE HOST -- hands a value back, copies from or to memory that may be pageable, waits for the stream, allocates or frees, times with events --
 *     and REFUSES while the context's stream is being captured: ECSIMD_HIP_ERR_BAD_ARG with "capture" in ecsimd_hip_last_error, decided BEFORE the
 *     stream is touched, so nothing is enqueued and the caller's capture stays valid (a synchronisation on a capturing stream would invalidate it).  These
 *     are sync, malloc, free, memcpy_h2d, memcpy_d2h, mask_count, scalar_mult_host, btc_merkle_root and peak_mad32;
 *   - it is no part of a stream's work and enqueues nothing on the context's stream: init, set / get_ref_square_compat, last_error, version, get_constant,
 *     register_modulus, register_curve, curve_capabilities, workspace_info, shard_range and the group_* family, whose groups own their contexts and
 *     streams -- and destroy, which WAITS for the context's stream before it frees what the context owns: it must not be called while that stream is
 *     being captured (the wait would invalidate the capture); end or abandon the capture first. */
int ecsimd_hip_set_stream(ecsimd_hip_ctx* ctx, void* hip_stream);
/* Go back to the non-blocking stream the context created in ecsimd_hip_init (the default). */
int ecsimd_hip_use_own_stream(ecsimd_hip_ctx* ctx);
/* Waits for the context's stream.  Refuses under stream capture (above). */
int ecsimd_hip_sync(ecsimd_hip_ctx* ctx);
/* Reference-square compatibility for every entry point that evaluates the reference's own expression DAG and contains a
 * squaring (square, mgry_sqr, mgry_pow, gfp_inverse, gfp_sqrt, compute_y, to_affine, DBLU ... TRPLU, the ladder):
 * on != 0 makes them square with mul.h:160-212 as written, dropped carry included (see ECSIMD_HIP_REF_SQUARE_COMPAT), and
 * walk exponents bit by bit as mgry_ops.h:44-86 does, so a caller gets the compiled reference's bits on every input.
 * Off by default.  The windowed algorithms are not the reference's and refuse to run while it is on. */
int ecsimd_hip_set_ref_square_compat(ecsimd_hip_ctx* ctx, int on);
/* The option as it stands: 0 / 1 (a caller that runs one job on two contexts mirrors it: integration/scalar_mult_p256_adapter.cpp); < 0: ctx is NULL. */
int ecsimd_hip_get_ref_square_compat(const ecsimd_hip_ctx* ctx);
const char* ecsimd_hip_last_error(const ecsimd_hip_ctx* ctx);
const char* ecsimd_hip_version(void);
/* Device memory on the context's device, and synchronous copies between it and host memory (pageable is fine: each copy has completed when the call
 * returns).  All four refuse under stream capture (above): allocate, fill and read back outside the capture. */
int ecsimd_hip_malloc(ecsimd_hip_ctx* ctx, void** dptr, size_t bytes);
int ecsimd_hip_free(ecsimd_hip_ctx* ctx, void* dptr);
int ecsimd_hip_memcpy_h2d(ecsimd_hip_ctx* ctx, void* dst, const void* src, size_t bytes);
int ecsimd_hip_memcpy_d2h(ecsimd_hip_ctx* ctx, void* dst, const void* src, size_t bytes);
/* device -> device on the context's stream (asynchronous, ordered with the kernels); what a by-value copy of a
 * reference `wide` (bignum.h:38-102: registers, copied freely) costs here when an in-out parameter is updated. */
int ecsimd_hip_memcpy_d2d(ecsimd_hip_ctx* ctx, void* dst, const void* src, size_t bytes);
/* Curve constants as the engine uses them (host memory, 4 x u64 each):
 * which = 0 p, 1 a, 2 b, 3 Gx, 4 Gy, 5 R mod p, 6 R^2 mod p, 7 -R mod p, 8 a*R, 9 b*R, 10 p-2, 11 (p+1)/4
 * (mgry_csts.h:15-24, curve_group.h:31-32, gfp.h:79-87). */
int ecsimd_hip_get_constant(int curve, int which, uint64_t out[4]);
/* A field id for the odd modulus p >= 3 (host pointer, 4 x u64 little-endian limbs): the host derives R mod p, R^2 mod p, -R mod p and m' = -p^-1 mod 2^32
 * (mgry_csts.h:15-35, mgry_mul.h:33-38) once; the element-wise field entry points then accept the id as `curve` (for a field id get_constant
 * reads zero in the curve slots 1-4, 8, 9).  The same (p, flags) gives the same id (the two curve primes give 0 / 1 whatever the flags); the same p with and
 * without MODULUS_PRIME are two ids, so that nobody's gfp_inverse changes under them; ids live as long as the process; thread-safe.  flags: 0 or ECSIMD_HIP_MODULUS_PRIME.  gfp_sqrt needs p = 3 mod 4, as the reference's GFp does (gfp.h:84). */
int ecsimd_hip_register_modulus(const uint64_t p[4], int flags, int* field_id);

/* A curve id for y^2 = x^3 + a x + b over GF(p) with generator (gx, gy) -- the reference's curve_group<Curve> instantiated with any Curve type that has
 * bn_type, P, A, B, Gx, Gy (curve.h:12-15; curve_group.h:25-33 derives Am, Bm from the type, :64-87 DBLU takes a from it, :91-218 the co-Z formulas and the
 * ladder are curve-independent) -- as a run-time registration: host pointers, 4 x u64 little-endian limbs, classical values < p.  p must be a prime with
 * p = 3 mod 4 (what the reference's GFp<WBN, P> needs: gfp.h:84) and the caller vouches for its primality; the generator must lie on the curve and the
 * curve must be non-singular (checked: ECSIMD_HIP_ERR_BAD_ARG).  n = the group order, or NULL (the reference has no order either: its ladder takes any
 * 256-bit k; with it the id gains the entry points listed below).  The id (>= ECSIMD_HIP_FIRST_REGISTERED_CURVE; the same parameters -- the order, or its
 * absence, included -- give the same id, so nobody's registration changes what an id somebody else holds does; P-256's or secp256k1's
 * parameters give 0 / 1 unless flags = ECSIMD_HIP_CURVE_GENERIC_KERNELS, which registers them like any other curve -- how tests hold the generic kernels
 * to the special-form ones bit for bit) is accepted by
 *     from_affine, to_affine, compute_y, on_curve, dblu, zaddu, zdau, add_z2_1, trplu, zdau_repeat, scalar_mult, scalar_mult_1s, scalar_mult_base, scalar_mult_host
 * (flags BASE_* | OUT_* | LADDER_RADIX32 | REF_SQUARE_COMPAT: the reference's ladder; of the table-driven algorithms a registered curve has all but the GLV split, all for
 * a curve registered with its order n >= 2^255 and all with OUT_AFFINE only: scalar_mult_base with ALG_WINDOWED -- a 4-bit odd-digit table of multiples of
 * ITS generator in LDS, built from the ladder on first use -- with ALG_WINDOWED | ALG_CONSTANT_TIME -- 5-bit windows, 52 x 16 odd multiples in 53 KB of LDS,
 * every entry of a window read and one kept under lane masks: SAFE for secret scalars -- or with ALG_WINDOWED_SIGNED -- signed 7-bit windows, 37 x 64 odd
 * multiples in 148 KiB of LDS, 36 additions instead of 63, public scalars (1.6 x the 4-bit comb) -- or with ALG_WINDOWED_BIG -- 20-bit windows, 13 x 2^19 odd
 * multiples in 436 MB of DEVICE memory per curve and context (built on first use: 0.3 s, 1.3 GB of temporary memory), 12 additions, public scalars (3.7 x) --
 * and scalar_mult / scalar_mult_1s with ALG_WINDOWED on a variable base --
 * the lane's own table of the eight odd multiples of P over one Z, 63 windows of three doublings and a fused double-add in modified Jacobian coordinates
 * on the isomorphic curve (any coefficient a; 640 B of context workspace per element, 2^22 at a time; 1.4 x the ladder's rate) -- public scalars: the table
 * is indexed by the scalar's digits; with ALG_CONSTANT_TIME every entry of the lane's table is read in every window and one kept under lane masks: SAFE for
 * secret scalars like the built-in curves' form (1.3 x the ladder).  The group must have prime order (cofactor 1: every valid point then has order n, which
 * is what "no addition inside the loop is exceptional" rests on) -- CHECKED at registration (n in p's Hasse interval, Miller-Rabin: ecsimd_hip_curve_capabilities);
 * an id without it keeps the ladder for a variable base (BAD_ARG for the flag, ladder passes inside double_scalar_mult / ecdsa_verify).
 * Either returns the true k P for every k, (0, 0) for k = 0 mod n.  The other ALG_* shapes exist for the two built-in curves only), by affine_add, sec1_encode, sec1_decode and -- when n was given, n >= 2^255, p < 2n, and
 * n - u is a good ladder scalar for u in {n - 1, 2^256 - n - 1, 2^256 - n} (every prime-order curve of this size) -- by double_scalar_mult,
 * ecdsa_verify_rx, ecdsa_verify, ecdsa_recover, ecdsa_sign, ecdsa_sign_recoverable: u1 G comes from the generator's signed comb -- from the 20-bit comb once that exists or the batch reaches 2^20 -- (sign: k G from the constant-time 5-bit comb), u2 Q (public) from the
 * lane's window table -- correct for every scalar in [0, n); ecdsa_sign's scratch is zeroed like the built-in curves'.  (Where an id has no comb or window table a
 * product is a pass of the ladder, the scalar kept clear of its three degenerate values: u -> n - u and the result negated.  n < 2^255: NO ECDSA -- BAD_ARG from
 * all of these.  There the ladder is wrong wherever u | 1 = 2^j mod n for a j from n's bit length to 256, not at three scalars: 2^192 - n and 2^192 - n - 1 on
 * P-192, hundreds on a 13-bit order; tools/ladder_degenerate_model.py)  Like the built-in curves', a call of
 * scalar_mult_base(OUT_AFFINE) without an algorithm flag on up to 2^16 lanes takes that comb (constant time) and returns the ladder's affine bits, its
 * three degenerate scalars included.  And, as a FIELD id, by every element-wise field entry point.  Same level-J parity as the built-in curves: X, Y, Z are
 * the bits the reference instantiated with this Curve returns.  The ladder's 254 iterations run on nine signed 29-bit limbs with the dense p in SGPRs
 * (81 multiply-adds per reduction where P-256's sparse form has 36); LADDER_RADIX32 / REF_SQUARE_COMPAT run them on 8 x 32-bit canonical words.
 * Process-wide, thread-safe, ids live as long as the process. */
enum { ECSIMD_HIP_CURVE_GENERIC_KERNELS = 1 };
/* What an id can do beyond the reference's layers (host only, no context): caps = a mask of
 *   HAS_ORDER (registered with n), COMB (ALG_WINDOWED [| ALG_CONSTANT_TIME] on its generator: n >= 2^255), ECDSA (double_scalar_mult, ecdsa_*: n >= 2^255, p < 2n and the
 *   ladder's three degenerate scalars have good images), WINDOW_VARIABLE_BASE (ALG_WINDOWED [| ALG_CONSTANT_TIME] on a variable base: n >= 2^255, n lies in p's Hasse
 *   interval -- so the group HAS order n -- and n passes Miller-Rabin: every point but infinity has order n).  The two built-in ids report all four.
 *   An n that passes those two tests and is NOT the generator's order (n G != O, checked once on the host: a neighbouring prime, a typo) gets HAS_ORDER
 *   alone: no COMB, no WINDOW_VARIABLE_BASE, no ECDSA.  A composite n, or one outside the Hasse interval, is taken on the caller's word for the
 *   generator's comb as before.  ECDSA also on an id whose n >= 2^255 fails the prime-order test: u2 Q then runs on the ladder, whose three-scalar
 *   work-around is complete for n >= 2^255. */
enum { ECSIMD_HIP_CURVE_HAS_ORDER = 1, ECSIMD_HIP_CURVE_COMB = 2, ECSIMD_HIP_CURVE_ECDSA = 4, ECSIMD_HIP_CURVE_WINDOW_VARIABLE_BASE = 8 };
int ecsimd_hip_curve_capabilities(int curve, int* caps);
int ecsimd_hip_register_curve(const uint64_t p[4], const uint64_t a[4], const uint64_t b[4], const uint64_t gx[4], const uint64_t gy[4],
                              const uint64_t n[4], int flags, int* curve_id);

/* ---- L2: bignum ops (curve independent) ----------------------------------------------- */
/* add.h:11-34  add: out = a + b mod 2^256, carry[i] = carry-out (carry may be NULL) */
int ecsimd_hip_add(ecsimd_hip_ctx*, const uint64_t* a, const uint64_t* b, uint64_t* out, uint8_t* carry, size_t n);
/* sub.h:12-38  sub: out = a - b mod 2^256, borrow[i] = borrow-out */
int ecsimd_hip_sub(ecsimd_hip_ctx*, const uint64_t* a, const uint64_t* b, uint64_t* out, uint8_t* borrow, size_t n);
/* sub.h:46-75  sub_if_above: out = a >= p ? a - p : a (p is per element, like the reference's wide p) */
int ecsimd_hip_sub_if_above(ecsimd_hip_ctx*, const uint64_t* a, const uint64_t* p, uint64_t* out, size_t n);
/* Lane masks on the device (the reference's eve::logical<wide>, bignum.h:136-137, with eve::all / eve::any):
 * cmp_eq: flag[i] = (a[i] == b[i]) over the low `limbs` (1..8) limbs of each element (element stride 4 limbs,
 * 8 for limbs > 4: a 128-bit value occupies the low half of a 256-bit element); mask_op: NOT (b ignored), AND, OR, EQ of
 * 0/1 byte masks; mask_count: number of non-zero flags (synchronises the stream: all = count == n, any = count > 0; refuses under stream capture). */
enum { ECSIMD_HIP_MASK_NOT = 0, ECSIMD_HIP_MASK_AND = 1, ECSIMD_HIP_MASK_OR = 2, ECSIMD_HIP_MASK_EQ = 3 };
int ecsimd_hip_cmp_eq(ecsimd_hip_ctx*, const uint64_t* a, const uint64_t* b, int limbs, uint8_t* flag, size_t n);
int ecsimd_hip_mask_op(ecsimd_hip_ctx*, int op, const uint8_t* a, const uint8_t* b, uint8_t* out, size_t n);
int ecsimd_hip_mask_count(ecsimd_hip_ctx*, const uint8_t* a, size_t n, size_t* count);
/* cmp.h:11-13  cmp_lt: flag[i] = a < b */
int ecsimd_hip_cmp_lt(ecsimd_hip_ctx*, const uint64_t* a, const uint64_t* b, uint8_t* flag, size_t n);
/* shift.h:13-32  shift_left_one: out = a << 1 mod 2^256, carry[i] = bit 255 of a */
int ecsimd_hip_shift_left_one(ecsimd_hip_ctx*, const uint64_t* a, uint64_t* out, uint8_t* carry, size_t n);
/* mul.h:150-158  mul: out8 = a * b (512 bits) */
int ecsimd_hip_mul(ecsimd_hip_ctx*, const uint64_t* a, const uint64_t* b, uint64_t* out8, size_t n);
/* mul.h:214-221  square: out8 = a * a */
int ecsimd_hip_square(ecsimd_hip_ctx*, const uint64_t* a, uint64_t* out8, size_t n);
/* swap.h:15-22  swap_if: swap a[i] and b[i] in place where mask[i] != 0 */
int ecsimd_hip_swap_if(ecsimd_hip_ctx*, const uint8_t* mask, uint64_t* a, uint64_t* b, size_t n);
/* ifelse.h:15-22  if_else: out[i] = mask[i] != 0 ? a[i] : b[i] (out may alias a or b) */
int ecsimd_hip_if_else(ecsimd_hip_ctx*, const uint8_t* mask, const uint64_t* a, const uint64_t* b, uint64_t* out, size_t n);

/* ---- wire formats on the device ------------------------------- */
/* serialization.h:12-24 bn_from_bytes_BE / :26-48 bn_to_bytes_BE over a batch: 32 big-endian bytes per
 * element <-> 4 x u64 little-endian limbs.  `bytes` is a device pointer, 16-byte aligned. */
int ecsimd_hip_from_bytes_be(ecsimd_hip_ctx*, const uint8_t* bytes, uint64_t* out, size_t n);
int ecsimd_hip_to_bytes_be(ecsimd_hip_ctx*, const uint64_t* in, uint8_t* bytes, size_t n);
/* The reference's own data format on the device (r5).  Its wide_bignum<bignum_256> is eve::wide<bignum, fixed<4>> -- four 256-bit lanes stored limb-major,
 * u64[limb * 4 + lane], 128 bytes (bignum.h:99-100; eve/arch/cpu/as_register.hpp:55-60) -- and a wide_jacobian_curve_point is three of them
 * (jacobian_curve_point.h:14-58).  A caller that keeps reference types copies its array of wides / points to the device as it is; these two do the 4 x 4
 * transposition there, at HBM speed, instead of a per-lane loop on the host: wide w of a record array (`record_bytes` apart, the wide at `offset_bytes`
 * inside its record: 128 / 0 for an array of wides; 384 / 0, 128, 256 for x, y, z of an array of Jacobian points) <-> elements 4w .. 4w + 3 of an ABI
 * array (u64[4 * e + limb]).  `wides` is a device pointer, 8-byte aligned; record_bytes and offset_bytes multiples of 8; not in place.
 * integration/scalar_mult_p256_adapter.cpp is the caller. */
int ecsimd_hip_wide4_to_lanes(ecsimd_hip_ctx*, const void* wides, size_t record_bytes, size_t offset_bytes, uint64_t* out, size_t n_wides);
int ecsimd_hip_lanes_to_wide4(ecsimd_hip_ctx*, const uint64_t* in, void* wides, size_t record_bytes, size_t offset_bytes, size_t n_wides);
/* utility.h:45-51 wide_mask_bit: flag[i] = bit `bit` (0..255, 0 = least significant) of a[i] */
int ecsimd_hip_mask_bit(ecsimd_hip_ctx*, const uint64_t* a, int bit, uint8_t* flag, size_t n);
/* SEC 1 v2 2.3.3: affine classical (x, y) -> 04||X||Y (65 B per point) or, compressed, 02/03||X (33 B). */
int ecsimd_hip_sec1_encode(ecsimd_hip_ctx*, int curve, const uint64_t* x, const uint64_t* y, uint8_t* out, size_t n, int compressed);
/* SEC 1 v2 2.3.4: the inverse.  ok[i] = 1 iff the record is well formed, x (and y) < p and the point is on
 * the curve (uncompressed) / x^3 + a x + b is a square (compressed: y recovered with the prefix's parity;
 * generalises curve_point_ops.h:12-22 from_x to per-lane validity and both curves).  The point at infinity
 * (single byte 00) has no fixed-size record and is not representable here. */
int ecsimd_hip_sec1_decode(ecsimd_hip_ctx*, int curve, const uint8_t* in, uint64_t* x, uint64_t* y, uint8_t* ok, size_t n, int compressed);

/* ---- L3: GF(p) ------------------------------------------------------------------------
 * `curve` is a FIELD id in this section (enum ecsimd_hip_field): a curve's prime or any registered modulus. */
/* modular.h:10-15 mod_add, :24-41 mod_sub, mgry_ops.h:14-22 mgry_shift_left<count> (1 <= count <= 255).
 * count | ECSIMD_HIP_SHIFT_FUSED runs pairs of doublings as one quadrupling with a single conditional subtraction (what the point
 * formulas use on their own intermediates): the same canonical residue for every a < p; for a >= p only the plain form is
 * the reference's chain of doublings. */
enum { ECSIMD_HIP_SHIFT_FUSED = 0x100 };
int ecsimd_hip_mod_add(ecsimd_hip_ctx*, int curve, const uint64_t* a, const uint64_t* b, uint64_t* out, size_t n);
int ecsimd_hip_mod_sub(ecsimd_hip_ctx*, int curve, const uint64_t* a, const uint64_t* b, uint64_t* out, size_t n);
int ecsimd_hip_mod_shift_left(ecsimd_hip_ctx*, int curve, const uint64_t* a, int count, uint64_t* out, size_t n);
/* Extension (the reference stops at mod_add / mod_sub, modular.h): classical a * b mod p, canonical. */
int ecsimd_hip_mod_mul(ecsimd_hip_ctx*, int curve, const uint64_t* a, const uint64_t* b, uint64_t* out, size_t n);
/* mgry_mul.h:84-121 details::mgry_reduce<P>: out = a8 * 2^-256 mod p (a8 < p * 2^256) */
int ecsimd_hip_mgry_reduce(ecsimd_hip_ctx*, int curve, const uint64_t* a8, uint64_t* out, size_t n);
/* mgry_ops.h:31-42 mgry_mul / mgry_sqr */
int ecsimd_hip_mgry_mul(ecsimd_hip_ctx*, int curve, const uint64_t* a, const uint64_t* b, uint64_t* out, size_t n);
int ecsimd_hip_mgry_sqr(ecsimd_hip_ctx*, int curve, const uint64_t* a, uint64_t* out, size_t n);
/* mgry.h:47-55 from_classical / to_classical */
int ecsimd_hip_mgry_from_classical(ecsimd_hip_ctx*, int curve, const uint64_t* a, uint64_t* out, size_t n);
int ecsimd_hip_mgry_to_classical(ecsimd_hip_ctx*, int curve, const uint64_t* a, uint64_t* out, size_t n);
/* mgry_ops.h:44-86 mgry_pow: out = a^e (Montgomery), e = ONE public exponent (host pointer, 4 x u64) */
int ecsimd_hip_mgry_pow(ecsimd_hip_ctx*, int curve, const uint64_t* a, const uint64_t exponent[4], uint64_t* out, size_t n);
/* gfp.h:42-44 inverse, :60-64 opposite, :46-54 sqrt.  sqrt reports validity PER ELEMENT in ok[]
 * (the reference collapses a wide to all-or-nothing; the C++ header reproduces that on top).  inverse shares one
 * inversion among up to 128 elements (Montgomery's trick) when out and a are different buffers; out == a inverts every
 * element on its own; 0 maps to 0 either way.  The inversion itself is the constant-time division-step ("safegcd") one,
 * not a^(p-2): the same unique inverse for every CANONICAL operand (a < p), which is what these two entry points take. */
int ecsimd_hip_gfp_inverse(ecsimd_hip_ctx*, int curve, const uint64_t* a, uint64_t* out, size_t n);
int ecsimd_hip_gfp_opposite(ecsimd_hip_ctx*, int curve, const uint64_t* a, uint64_t* out, size_t n);
int ecsimd_hip_gfp_sqrt(ecsimd_hip_ctx*, int curve, const uint64_t* a, uint64_t* out, uint8_t* ok, size_t n);

/* ---- L4/L5: points and the group ------------------------------------------------------ */
/* jacobian_curve_point.h:25-31 from_affine (Z := R mod p), :33-42 to_affine.  to_affine uses Montgomery's
 * simultaneous inversion (one shared inversion per up to 128 elements (k_affine.inc BATCH_INVERSION_MAX); identical values) unless x/y alias the inputs.
 * to_affine: y may be NULL (the x coordinate only: 5 field multiplications per element instead of 7). */
int ecsimd_hip_from_affine(ecsimd_hip_ctx*, int curve, const uint64_t* x, const uint64_t* y, uint64_t* jx, uint64_t* jy, uint64_t* jz, size_t n);
int ecsimd_hip_to_affine(ecsimd_hip_ctx*, int curve, const uint64_t* jx, const uint64_t* jy, const uint64_t* jz, uint64_t* x, uint64_t* y, size_t n);
/* curve_group.h:43-58 compute_y for y^2 = x^3 + a x + b (classical in/out), per-element ok[] */
int ecsimd_hip_compute_y(ecsimd_hip_ctx*, int curve, const uint64_t* x, uint64_t* y, uint8_t* ok, size_t n);
/* curve_group.h:64-87 DBLU: r = 2P, P rewritten in place with r's Z.  P.z must be mgry(1).
 * (DBLU, ZADDU, ZDAU, TRPLU: co-Z, ONE Z for the result and the rewritten operand -- rz may be the very array pz (ZDAU: qz); it is then written once.)
 * Point formulas and the ladder take CANONICAL coordinates (< p), which is what every entry point of this library returns; the element-wise
 * field operations above additionally reproduce the reference on operands >= p (it never rejects them, tests/ops.cpp:232). */
int ecsimd_hip_dblu(ecsimd_hip_ctx*, int curve, uint64_t* px, uint64_t* py, uint64_t* pz, uint64_t* rx, uint64_t* ry, uint64_t* rz, size_t n);
/* curve_group.h:91-116 ZADDU: r = P + O (co-Z), P rewritten in place with r's Z. */
int ecsimd_hip_zaddu(ecsimd_hip_ctx*, int curve, uint64_t* px, uint64_t* py, uint64_t* pz, const uint64_t* ox, const uint64_t* oy, const uint64_t* oz, uint64_t* rx, uint64_t* ry, uint64_t* rz, size_t n);
/* curve_group.h:120-153 ZDAU: r = 2P + Q (co-Z), Q rewritten in place with r's Z. */
int ecsimd_hip_zdau(ecsimd_hip_ctx*, int curve, const uint64_t* px, const uint64_t* py, const uint64_t* pz, uint64_t* qx, uint64_t* qy, uint64_t* qz, uint64_t* rx, uint64_t* ry, uint64_t* rz, size_t n);
/* Diagnostic / micro-benchmark (r4): ZDAU applied `iters` times IN REGISTERS -- the ladder's loop body alone (curve_group.h:206-210 without the
 * scalar): per iteration (P, Q) <- (2P + Q, Q re-expressed with the new Z), and after iteration t the two outputs are exchanged where bit
 * (t mod 64) of `swap_bits` is set.  (rx, ry) = the final P, (sx, sy) = the final Q, oz their Z; all Montgomery form, canonical.
 * radix = 32: on field.cuh's 8 x 32-bit canonical words (rounds 1-3); radix = 29: on fe29.cuh's nine signed 29-bit limbs, the representation
 * the ladder's loop runs in since round 4 -- the SAME field values, so the same bits out (tests/test_gpu_parity.py pins both to the oracle's
 * ZDAU iterated on the CPU).  Not available with the reference-square option for radix 29. */
int ecsimd_hip_zdau_repeat(ecsimd_hip_ctx*, int curve, const uint64_t* px, const uint64_t* py, const uint64_t* pz, const uint64_t* qx, const uint64_t* qy,
                           uint64_t* rx, uint64_t* ry, uint64_t* sx, uint64_t* sy, uint64_t* oz, size_t n, int iters, uint64_t swap_bits, int radix);
/* curve_group.h:155-179 ADD_Z2_1: r = A + B with B = (bx, by) Montgomery-form affine (Z2 = mgry(1)). */
int ecsimd_hip_add_z2_1(ecsimd_hip_ctx*, int curve, const uint64_t* ax, const uint64_t* ay, const uint64_t* az, const uint64_t* bx, const uint64_t* by, uint64_t* rx, uint64_t* ry, uint64_t* rz, size_t n);
/* Extension: the complete form of the mixed addition -- r = A + B for every input: A = infinity (Z = 0), B = infinity
 * ((0, 0)), A = B (tangent), A = -B (r = infinity: Z = 0).  Same conventions as add_z2_1 (B Montgomery-form affine);
 * r is a representative of the same point as ADD_Z2_1's where that formula is defined (Z3 = Z1*H instead of 2*Z1*H). */
int ecsimd_hip_add_mixed_complete(ecsimd_hip_ctx*, int curve, const uint64_t* ax, const uint64_t* ay, const uint64_t* az, const uint64_t* bx, const uint64_t* by, uint64_t* rx, uint64_t* ry, uint64_t* rz, size_t n);
/* curve_group.h:183-186 TRPLU: r = 3P, P rewritten in place with r's Z.  P.z must be mgry(1). */
int ecsimd_hip_trplu(ecsimd_hip_ctx*, int curve, uint64_t* px, uint64_t* py, uint64_t* pz, uint64_t* rx, uint64_t* ry, uint64_t* rz, size_t n);

/* curve_group.h:189-218 scalar_mult (per-element scalar k[i], per-element base point (x[i], y[i])):
 * the co-Z Joye double-add ladder of the reference, any 256-bit k.  flags = BASE_* | OUT_*, optionally
 * OUT_AFFINE | ALG_WINDOWED for the faster windowed algorithm (affine-level parity, see the flag). */
int ecsimd_hip_scalar_mult(ecsimd_hip_ctx*, int curve, const uint64_t* k, const uint64_t* x, const uint64_t* y,
                           uint64_t* ox, uint64_t* oy, uint64_t* oz, size_t n, int flags);
/* curve_group.h:221-251 scalar_mult_1s: ONE scalar (host pointer) for all points; flags as for scalar_mult. */
int ecsimd_hip_scalar_mult_1s(ecsimd_hip_ctx*, int curve, const uint64_t k1[4], const uint64_t* x, const uint64_t* y,
                              uint64_t* ox, uint64_t* oy, uint64_t* oz, size_t n, int flags);
/* curve_group.h:35-41 WJG + scalar_mult: k[i] * G (base = the curve generator); ecsimd_hip_scalar_mult with x = y = NULL and ECSIMD_HIP_BASE_GENERATOR is the same call.
 * Small batches (r4): with OUT_AFFINE, no ALG_* / REF_SQUARE_COMPAT / LADDER_RADIX32 flag and n <= 2^16 the product comes from the constant-time
 * 5-bit comb (ALG_WINDOWED | ALG_CONSTANT_TIME's kernel: as safe for secret scalars as the ladder) instead of a 254-iteration ladder launch whose
 * cost does not depend on n -- 0.2 ms instead of 1.3 ms -- with the SAME affine bits: at the ladder's three degenerate scalars (n - 1,
 * 2^256 - n - 1, 2^256 - n) the lanes take the ladder's own coordinates by select.  The first such call per curve builds the comb's table. */
int ecsimd_hip_scalar_mult_base(ecsimd_hip_ctx*, int curve, const uint64_t* k, uint64_t* ox, uint64_t* oy, uint64_t* oz, size_t n, int flags);
/* Extensions built on the kernels above (not in the reference):
 * affine_add: R = A + B for affine classical points, one shared inversion per up to 128 points (Montgomery's trick).  (0, 0) encodes the point
 * at infinity on input and output; finite[i] = 0 marks an infinite result (finite and ry may be NULL; rx must
 * not alias an input). */
int ecsimd_hip_affine_add(ecsimd_hip_ctx*, int curve, const uint64_t* ax, const uint64_t* ay, const uint64_t* bx, const uint64_t* by,
                          uint64_t* rx, uint64_t* ry, uint8_t* finite, size_t n);
/* on_curve: ok[i] = x[i], y[i] < p and y^2 = x^3 + a x + b (classical coordinates) -- SEC 1 public-key validation (both
 * curves have cofactor 1); (0, 0), this library's point at infinity, fails. */
int ecsimd_hip_on_curve(ecsimd_hip_ctx*, int curve, const uint64_t* x, const uint64_t* y, uint8_t* ok, size_t n);
/* double_scalar_mult: R[i] = u1[i]*G + u2[i]*Q[i], affine classical (the ECDSA-verification shape; pass
 * ry = NULL for x only).  u1*G uses the windowed fixed-base kernel, u2*Q the windowed variable-base kernels
 * (ALG_WINDOWED): correct for every 256-bit u1, u2; 1 632 B of context workspace per element, 2^22 at a time.
 * Q[i] is VALIDATED (on_curve): an invalid public key -- off the curve, a coordinate >= p, the point at infinity --
 * gives R[i] = (0, 0) and finite[i] = 0.  The scalars here are public (signature verification): the window kernels index
 * their tables by scalar digits and are not for secret scalars.  u1*G goes through the 436 MB table of 20-bit windows once it
 * exists in this context or n >= 2^16 (which builds it); smaller batches use the 148 KiB table in LDS and keep nothing that size. */
int ecsimd_hip_double_scalar_mult(ecsimd_hip_ctx*, int curve, const uint64_t* u1, const uint64_t* u2, const uint64_t* qx, const uint64_t* qy,
                                  uint64_t* rx, uint64_t* ry, uint8_t* finite, size_t n);
/* (ok[i] is also 0 when Q[i] fails the validation above.)  The acceptance test of an ECDSA verification for precomputed u1 = e/s, u2 = r/s (mod n; ecsimd_hip_ecdsa_verify
 * below computes them on the device): ok[i] = 1 iff u1[i]*G + u2[i]*Q[i] is a finite point whose
 * x coordinate, reduced mod n, equals r[i].  Same workspace as double_scalar_mult plus 33 B per element. */
int ecsimd_hip_ecdsa_verify_rx(ecsimd_hip_ctx*, int curve, const uint64_t* u1, const uint64_t* u2, const uint64_t* qx, const uint64_t* qy,
                               const uint64_t* r, uint8_t* ok, size_t n);
/* ECDSA verification of n signatures (SEC 1 v2 4.1.4, FIPS 186-5 6.4.2; not in the reference -- SURVEY.md 8(f) rank 4, "the first real application of the
 * engine").  Per element, all classical 4 x u64 LE limbs in device memory: e = the message digest as an integer (its leftmost 256 bits; ANY 256-bit value is
 * taken and reduced mod n), (r, s) = the signature, (qx, qy) = the public key.  ok[i] = 1 iff 1 <= r, s < n, Q is a valid public key (on_curve), and
 * R = (e/s) G + (r/s) Q is a finite point with x(R) mod n == r.  The arithmetic modulo the group order n runs on the device (field id
 * ECSIMD_HIP_FIELD_*_ORDER: generic Montgomery multiplication, one constant-time division-step inversion shared by up to 128 signatures), then
 * ecdsa_verify_rx's kernels.  Public data only (the window kernels index tables by scalar digits).  Workspace: ecdsa_verify_rx's plus 65 B per element. */
int ecsimd_hip_ecdsa_verify(ecsimd_hip_ctx*, int curve, const uint64_t* e, const uint64_t* r, const uint64_t* s, const uint64_t* qx, const uint64_t* qy,
                            uint8_t* ok, size_t n);
/* ECDSA signing of n digests (SEC 1 v2 4.1.3; not in the reference): e = the digest as an integer, d = the private key, k = the per-signature nonce --
 * the CALLER's here (a DRBG's, or RFC 6979's: ecsimd_hip_rfc6979_nonce / ecsimd_hip_ecdsa_sign_deterministic below make that one on the device; this
 * library has no random source), 1 <= d, k < n.  R = k G comes from the constant-time comb (the kernel
 * of ALG_WINDOWED | ALG_CONSTANT_TIME), r = x(R) mod n, s = k^-1 (e + r d) mod n on the device (generic Montgomery products on the order's field id, one
 * constant-time division-step inversion shared by up to 128 signatures).  ok[i] = 1 and (r, s) a valid signature, or ok[i] = 0 and r = s = 0 where d or k is
 * out of range or r or s came out 0 (probability ~2^-255: sign again with another nonce).  d and k are treated as SECRETS: no branch or address depends on
 * them, checked on the shipped ISA: the comb's window loop by tools/ct_check.py check(), and the comb as a whole, the x-only simultaneous inversion of k G and
 * the scalar-field kernel (its division-step inversion included) by check_secret_flow, a taint analysis from the loads of d, k and k G to every branch
 * condition, lane mask in force at a memory access, and address (tests/test_constant_time_isa.py).  The Jacobian k G and its x are zeroed in the context
 * workspace on the stream before the call returns.  r, s must not alias an input.  Workspace: 128 B per element. */
int ecsimd_hip_ecdsa_sign(ecsimd_hip_ctx*, int curve, const uint64_t* e, const uint64_t* d, const uint64_t* k, uint64_t* r, uint64_t* s, uint8_t* ok, size_t n);
/* Public-key recovery from n signatures (SEC 1 v2 4.1.6; not in the reference): the operation behind Ethereum-style transaction checking.  e, r, s as in
 * ecdsa_verify (e is ANY 256-bit value, reduced mod n); v[i] = the recovery id, one byte per element: bit 0 = the parity of y(R), bit 1 = x(R) was >= n,
 * R = k G of the signer.  Per element, with x = r + (v >> 1) n:  ok[i] = 1 iff v <= 3, 1 <= r, s < n, x < p, x^3 + a x + b is a square modulo p, and
 * Q = (-e/r) G + (s/r) R is a finite point, R = (x, y) with y the root whose parity is v & 1.  Where ok[i] = 0, qx = qy = 0 (this library's point at infinity).
 * qy may be NULL (x only).  One pass modulo p lifts r to R, one pass modulo n forms the two scalars (one constant-time division-step inversion of r shared by up
 * to 128 signatures), then double_scalar_mult's window loops WITHOUT its validation of the point: R was just built from the curve equation.  Public data only
 * (signatures and digests; the window kernels index tables by scalar digits and are not for secret scalars).  Any n (2^22 at a time through the window loops).
 * Workspace: double_scalar_mult's plus 129 B per element. */
int ecsimd_hip_ecdsa_recover(ecsimd_hip_ctx*, int curve, const uint64_t* e, const uint64_t* r, const uint64_t* s, const uint8_t* v,
                             uint64_t* qx, uint64_t* qy, uint8_t* ok, size_t n);
/* ecdsa_sign that also returns the recovery id: r, s, ok, the range checks, the aliasing rule and the treatment of d and k as SECRETS are ecdsa_sign's, bit for bit
 * with flags = 0.  v[i] = parity(y(k G)) | (x(k G) >= n ? 2 : 0), and 0 where ok[i] = 0.  flags = ECSIMD_HIP_ECDSA_LOW_S: where s > n / 2 (integer halving) the call
 * returns n - s and flips bit 0 of v (the canonical form Bitcoin and Ethereum ask for; still a valid signature of the same key).  y(k G) comes out of the same
 * simultaneous inversion as x; v and the low-s rule are formed by selects only (tools/ct_check.py check_secret_flow on the shipped ISA, from the loads of the
 * affine k G and of s: tests/test_ecdsa_recover_cpu.py) -- r, s and v are public once returned, a refused lane gives nothing away.  The Jacobian k G and BOTH its
 * affine coordinates are zeroed in the context workspace on the stream before the call returns.  Workspace: 160 B per element. */
enum { ECSIMD_HIP_ECDSA_LOW_S = 1 };
int ecsimd_hip_ecdsa_sign_recoverable(ecsimd_hip_ctx*, int curve, const uint64_t* e, const uint64_t* d, const uint64_t* k, uint64_t* r, uint64_t* s, uint8_t* v, uint8_t* ok,
                                      size_t n, int flags);
/* SHA-256 (FIPS 180-4) of n messages of msg_bytes bytes each, message i at msg + i * stride_bytes (stride_bytes >= msg_bytes; device memory, any alignment --
 * a base and a stride that are multiples of 4 are read a word at a time).  e[i] = SHA-256(message i) as the integer the ECDSA calls take: 4 x u64 little-endian
 * limbs of the digest read as a big-endian number.  Public data.  msg_bytes = 0 is allowed (msg may then be NULL).  One message per lane, the state and the
 * message schedule in registers; equal lengths only (one length per lane: ecsimd_hip_sha256_lens, with Bitcoin's hashes below). */
int ecsimd_hip_sha256(ecsimd_hip_ctx*, const uint8_t* msg, size_t msg_bytes, size_t stride_bytes, uint64_t* e, size_t n);
/* The deterministic nonce of RFC 6979 section 3.2 with H = SHA-256 (HMAC-SHA-256), bit for bit: k[i] for digest e[i] and private key d[i].  Supported where
 * qlen = 256, i.e. the group order n >= 2^255: the two built-in curves and every registered curve with the ECDSA capability and such an order (brainpoolP256r1,
 * SM2, FRP256v1, ...); any other curve id is ECSIMD_HIP_ERR_BAD_ARG.  e is ANY 256-bit value, as in the other ECDSA calls: h1 = its 32 big-endian bytes,
 * bits2octets(h1) = e - n where e >= n; RFC 6979 proper when e is a SHA-256 digest, and for another 256-bit digest what libsecp256k1 does.  ok[i] = 0 and
 * k[i] = 0 where d is not in [1, n - 1].  d, the HMAC state (K, V), every candidate and k are SECRETS: no branch, address or lane mask in force at a memory
 * access depends on them (tools/ct_check.py check_secret_flow on the shipped ISA: tests/test_ecdsa_deterministic_cpu.py) -- with the one exception RFC 6979
 * itself makes: step h.3 loops while a candidate is outside [1, n - 1].  That one bit per candidate passes through a byte array of its own in the workspace,
 * written by the first kernel and re-read as public data by the retry kernel; a rejected candidate says nothing about the accepted one.  A lane may try
 * C(n) candidates, C(n) = ceil(128 / -log2(1 - n / 2^256)) evaluated in double precision when the curve is looked up (secp256k1 2, P-256 4, SM2 4, FRP256v1 31,
 * brainpoolP256r1 82); a lane that exhausts them gets ok[i] = 0, k[i] = 0: probability (1 - n / 2^256)^C(n) <= 2^-128 per lane (SM2, whose 2^256 - n rounds to
 * 2^224: 2^-128 (1 + 2^-95)).  16 SHA-256 compressions per lane and 8 per further candidate (the HMAC key midstates are kept).  Everything is stream-ordered;
 * nothing is read back.  K, V and the retry bytes are zeroed in the workspace on the stream before the call returns.  k must not alias an input.  Any n (2^22
 * at a time).  Workspace: 130 B per element. */
int ecsimd_hip_rfc6979_nonce(ecsimd_hip_ctx*, int curve, const uint64_t* e, const uint64_t* d, uint64_t* k, uint8_t* ok, size_t n);
/* ecdsa_sign_recoverable with k = the RFC 6979 nonce of (e, d), never seen by the caller: the nonce kernels write k into the context workspace, then exactly
 * the kernels of ecdsa_sign_recoverable run, so r, s, v, ok are those of the chain rfc6979_nonce -> ecdsa_sign_recoverable bit for bit, on every curve and
 * flag (ECSIMD_HIP_ECDSA_LOW_S).  v may be NULL.  Curves, the treatment of d and k as SECRETS, the cap on candidates and its probability: as for
 * ecsimd_hip_rfc6979_nonce; ranges and aliasing: as for ecdsa_sign_recoverable.  ONE deviation from RFC 6979: where r or s comes out 0 (probability ~2^-255)
 * the lane gets ok = 0, as in ecdsa_sign, instead of the next candidate.  K, V, the candidates and the nonce are zeroed in the workspace on the stream before
 * the call returns, the Jacobian k G and its affine coordinates as in ecdsa_sign_recoverable.  Any n (2^22 at a time).  Workspace: ecdsa_sign_recoverable's
 * (160 B per element on the built-in curves, 290 B on a registered one) plus 130 B per element. */
int ecsimd_hip_ecdsa_sign_deterministic(ecsimd_hip_ctx*, int curve, const uint64_t* e, const uint64_t* d, uint64_t* r, uint64_t* s, uint8_t* v, uint8_t* ok,
                                        size_t n, int flags);
/* BIP-340 Schnorr signatures (Bitcoin Taproot, Nostr).  Defined for secp256k1 only: no curve id, ECSIMD_HIP_SECP256K1 throughout.  Keys, r, s and aux are 4 x u64
 * little-endian limbs per element like everything else (the integer whose 32 big-endian bytes the BIP writes); message i lies at msg + i * stride_bytes and is
 * msg_bytes long, as for ecsimd_hip_sha256 (any length including 0, msg may then be NULL; any alignment, word loads where base and stride are multiples of 4).
 * Tagged hashes start from the midstate of their tag block, a constant: with 32-byte messages a challenge or nonce hash is two SHA-256 compressions, the aux hash
 * one.  Stream-ordered, nothing is read back.  No ECSIMD_HIP_REF_SQUARE_COMPAT form (ERR_BAD_ARG on a context with that option).  Any n (2^22 at a time).
 *
 * Verify (BIP-340 "Verify"), PUBLIC data: ok[i] = 1 iff px < p and lifts to the even-y point P, r < p, s < n, and R = s G - e P is finite, has even y and
 * x(R) == r, with e = int(SHA256(tag || tag || bytes(r) || bytes(px) || m)) mod n, tag = SHA256("BIP0340/challenge").  One kernel hashes, lifts and range-checks
 * (no inversion modulo n, unlike ECDSA), double_scalar_mult's window loops form the sum (indexed by scalar digits: not for secrets), one kernel accepts.
 * Workspace: double_scalar_mult's plus 194 B per element of a chunk. */
int ecsimd_hip_schnorr_verify(ecsimd_hip_ctx*, const uint64_t* px, const uint8_t* msg, size_t msg_bytes, size_t stride_bytes,
                              const uint64_t* r, const uint64_t* s, uint8_t* ok, size_t n);
/* Sign (BIP-340 "Default Signing", bit for bit): d = the secret key, aux = 32 bytes of auxiliary randomness per element as an integer (big-endian bytes = the
 * BIP's aux_rand), or NULL = 32 zero bytes (what libsecp256k1 does for a null aux_rand32).  px (optional output, may be NULL) = x(d G), the x-only public key.
 * ok[i] = 0 and r = s = px = 0 where d is not in [1, n - 1] or the nonce came out 0 (probability 2^-256).  The signature is not re-verified: a caller who wants the
 * BIP's recommended check calls ecsimd_hip_schnorr_verify on the result.  d, aux, d' (d or n - d), t, the nonce hash, the nonce k0, k, the Jacobian and the affine
 * d G and k0 G are SECRETS until returned: both products run on the constant-time comb (the kernel of ALG_WINDOWED | ALG_CONSTANT_TIME) and the select-only
 * simultaneous inversion, the two kernels around them select by masks -- no branch, address or lane mask in force at a memory access depends on a secret, and
 * unlike RFC 6979 no bit is declassified (tools/ct_check.py check_secret_flow on the shipped ISA: tests/test_schnorr_cpu.py).  Every workspace byte the call
 * used is zeroed on the stream before it returns.  r, s and px must not alias an input or each other.  Workspace: 256 B per element of a chunk. */
int ecsimd_hip_schnorr_sign(ecsimd_hip_ctx*, const uint64_t* d, const uint8_t* msg, size_t msg_bytes, size_t stride_bytes,
                            const uint64_t* aux, uint64_t* px, uint64_t* r, uint64_t* s, uint8_t* ok, size_t n);
/* Keccak-256 as Ethereum uses it: the original Keccak padding (pad byte 0x01, final bit 0x80, rate 136), NOT NIST's SHA-3 (pad byte 0x06).  Message i lies at
 * msg + i * stride_bytes (device memory, any alignment: 8-byte loads where base and stride are multiples of 8, 4-byte loads where they are multiples of 4, byte
 * loads otherwise).  lens = NULL: every message is msg_bytes long (stride_bytes >= msg_bytes; 0 is allowed, msg may then be NULL) and every branch is uniform.
 * lens != NULL (n x u32, device memory): lane i absorbs lens[i] bytes, lens[i] <= stride_bytes (a larger value is read as stride_bytes), msg_bytes is ignored and
 * the block loop runs per lane.  Any length, any number of blocks.  e[i] = the digest as the integer the ECDSA calls take, as ecsimd_hip_sha256 writes it: 4 x u64
 * little-endian limbs of the digest read as a big-endian number.  PUBLIC data: the loads and the loop follow the message lengths; do not hash a secret with it.
 * One message per lane, the 25 lanes of the state in registers, the 24 rounds unrolled.  Stream-ordered; no workspace. */
int ecsimd_hip_keccak256(ecsimd_hip_ctx*, const uint8_t* msg, size_t msg_bytes, size_t stride_bytes, const uint32_t* lens, uint64_t* e, size_t n);
/* Ethereum addresses of n public keys: addr[20 i .. 20 i + 19] = the last 20 bytes of Keccak-256(be32(qx[i]) || be32(qy[i])), one permutation per lane.  No
 * validation: the call hashes the 64 bytes it is given (for the point at infinity (0, 0) that is the address of 64 zero bytes).  addr: device memory, 4-byte
 * aligned.  PUBLIC data.  Stream-ordered; no workspace.  (The address of a SECRET key d: ecsimd_hip_scalar_mult_base with ECSIMD_HIP_ALG_WINDOWED |
 * ECSIMD_HIP_ALG_CONSTANT_TIME | ECSIMD_HIP_OUT_AFFINE, then this call on the public result.) */
int ecsimd_hip_eth_address(ecsimd_hip_ctx*, const uint64_t* qx, const uint64_t* qy, uint8_t* addr, size_t n);
/* Ethereum's ecrecover over n signatures: the sender's address straight from (e, r, s, v), secp256k1 only (no curve id).  e is any 256-bit value (for a
 * transaction: ecsimd_hip_keccak256 of its signing bytes).  v[i] must be 0, 1, 27 or 28; 27 and 28 mean 0 and 1; every other value is refused -- ecdsa_recover's
 * 2 and 3 included: Ethereum does not accept x(R) >= n.  ok[i] = 1 iff v[i] is accepted and ecsimd_hip_ecdsa_recover with that recovery id (0 or 1) sets it;
 * flags = ECSIMD_HIP_ETH_REQUIRE_LOW_S additionally asks s <= n / 2 (EIP-2).  addr as for ecsimd_hip_eth_address; where ok[i] = 0 it is 20 zero bytes and
 * qx = qy = 0.  qx and qy are optional outputs (NULL, or both given): with NULL the recovered key stays in the context workspace and never reaches caller memory.
 * Per chunk of 2^22 lanes: one kernel maps v (and the low-s rule) to a recovery id or to the value the lift refuses, then ecdsa_recover's own kernels -- the lift,
 * the scalars modulo n, the window loops without re-validation -- then the address kernel on the affine result.  Stream-ordered, nothing is read back.  PUBLIC
 * data only.  No ECSIMD_HIP_REF_SQUARE_COMPAT form (ERR_BAD_ARG on a context with that option).  Any n.  Workspace: double_scalar_mult's plus 194 B per element of
 * a chunk (ecdsa_recover's 129, the key's 64, the recovery id's 1). */
enum { ECSIMD_HIP_ETH_REQUIRE_LOW_S = 1 };
int ecsimd_hip_eth_recover(ecsimd_hip_ctx*, const uint64_t* e, const uint64_t* r, const uint64_t* s, const uint8_t* v,
                           uint8_t* addr, uint64_t* qx, uint64_t* qy, uint8_t* ok, size_t n, int flags);
/* Bitcoin's hashes over n equal-length messages, message i at msg + i * stride_bytes, msg_bytes long, as for ecsimd_hip_sha256: any length including 0 (msg may
 * then be NULL), stride_bytes >= msg_bytes, any alignment (word loads where base and stride are multiples of 4, byte loads otherwise).  PUBLIC data: the loads
 * and the block loop follow the length; do not hash a secret with these.  out20: n x 20 bytes of device memory, 4-byte aligned: lane i's digest at out20 + 20 i,
 * its bytes in order.  Stream-ordered; no workspace.  One message per lane; RIPEMD-160's five state words and sixteen message words stay in registers, its
 * 80 + 80 steps are unrolled.
 *   ripemd160   RIPEMD-160(m).
 *   hash160     RIPEMD-160(SHA-256(m)): what a P2PKH / P2WPKH output holds of a key, a P2SH output of a script.  The SHA-256 digest enters the RIPEMD block in
 *               registers: c + 1 compressions for a message of c SHA-256 blocks.
 *   sha256d     SHA-256(SHA-256(m)): transaction ids, legacy and segwit-v0 signature hashes, Base58Check checksums.  e[i] = the digest as ecsimd_hip_sha256
 *               writes it: 4 x u64 little-endian limbs of the digest read as a big-endian number (16-byte aligned).  c + 1 compressions. */
int ecsimd_hip_ripemd160(ecsimd_hip_ctx*, const uint8_t* msg, size_t msg_bytes, size_t stride_bytes, uint8_t* out20, size_t n);
int ecsimd_hip_hash160(ecsimd_hip_ctx*, const uint8_t* msg, size_t msg_bytes, size_t stride_bytes, uint8_t* out20, size_t n);
int ecsimd_hip_sha256d(ecsimd_hip_ctx*, const uint8_t* msg, size_t msg_bytes, size_t stride_bytes, uint64_t* e, size_t n);
/* The same four hashes -- ecsimd_hip_sha256 and the three above -- with one length per lane, for transactions, scripts and witness items, which never share one:
 * lens as in ecsimd_hip_keccak256.  lens != NULL (n x u32, device memory, 4-byte aligned): lane i hashes the first min(lens[i], stride_bytes) bytes of its row,
 * msg_bytes is ignored and the block loop runs per lane, so a wave runs until its longest lane is done.  lens == NULL: exactly the equal-length call, which is
 * called.  No byte at or behind a lane's message is loaded: the last row need only be lens[n - 1] bytes long.  stride_bytes = 0 with n > 1 is refused (every lane
 * would read lane 0's row).  Word loads where base and stride are multiples of 4, byte loads otherwise; the last one or two blocks are padded in registers.
 * ECSIMD_HIP_REF_SQUARE_COMPAT does not concern these calls (no curve arithmetic).  PUBLIC data.  Stream-ordered; no workspace. */
int ecsimd_hip_sha256_lens(ecsimd_hip_ctx*, const uint8_t* msg, size_t msg_bytes, size_t stride_bytes, const uint32_t* lens, uint64_t* e, size_t n);
int ecsimd_hip_sha256d_lens(ecsimd_hip_ctx*, const uint8_t* msg, size_t msg_bytes, size_t stride_bytes, const uint32_t* lens, uint64_t* e, size_t n);
int ecsimd_hip_hash160_lens(ecsimd_hip_ctx*, const uint8_t* msg, size_t msg_bytes, size_t stride_bytes, const uint32_t* lens, uint8_t* out20, size_t n);
int ecsimd_hip_ripemd160_lens(ecsimd_hip_ctx*, const uint8_t* msg, size_t msg_bytes, size_t stride_bytes, const uint32_t* lens, uint8_t* out20, size_t n);
/* The Merkle roots of m trees of txids (or wtxids) in one call, by Bitcoin Core's ComputeMerkleRoot: level by level, node j = SHA256d(be32(L[2j]) || be32(L[2j + 1])),
 * the last node paired with itself where the level's count is odd; a tree of one leaf is that leaf.  Tree t's leaves are leaves[tree_offsets[t] ..
 * tree_offsets[t + 1]) in device memory (4 x u64 limbs each, as ecsimd_hip_sha256d returns txids, 16-byte aligned); tree_offsets: m + 1 non-decreasing u64 in
 * HOST memory (the counts are public, and the host sizes every level with them), read before the call returns.  An empty tree is ECSIMD_HIP_ERR_BAD_ARG; m = 0
 * succeeds.  roots: m x 4 limbs.  mutated (m bytes of device memory, or NULL): mutated[t] = 1 iff on any level a REAL pair (2j + 1 < count) holds two equal
 * values, else 0 -- Bitcoin Core's flag for CVE-2012-2459, evaluated before the last node is duplicated.  One launch per level, one lane per parent node
 * across all trees: the lane finds its tree by bisection over the level's node offsets, which the host computes for all levels at once and uploads in one
 * stream-ordered copy from a pinned block of the context (a second call waits for the first one's copy, not for its kernels' results; the host work makes
 * the call refuse under stream capture).  Three compressions per
 * parent; the padding block's schedule is a constant.  Trees are taken in chunks of whole trees with at most 2^22 first-level parents (a larger tree is a chunk
 * of its own).  PUBLIC data.  Stream-ordered, nothing read back.  Workspace, per chunk: 32 B per parent of the first level and of the second (the levels
 * ping-pong) -- 24 B per leaf for large trees, at most 64 B per leaf --, and 8 B x (trees + 1) x (levels + 1) of offsets for every chunk of the call. */
int ecsimd_hip_btc_merkle_root(ecsimd_hip_ctx*, const uint64_t* leaves, const uint64_t* tree_offsets, size_t m, uint64_t* roots, uint8_t* mutated);
/* BIP-341 script paths, PUBLIC data.  With them and ecsimd_hip_taproot_tweak_pubkey a script-path spend is checked without leaving the device: the leaf hash of
 * the script, the walk up the control block's path to the merkle root, the tweak of the internal key by it, and the comparison of qx and parity with the
 * output key and the control byte's low bit (ecsimd_hip_cmp_eq).  Stream-ordered; no workspace; nothing read back.
 *
 * tapleaf_hash: e[i] = SHA256(tag || tag || version || compact_size(len) || script), tag = SHA256("TapLeaf"), from the tag block's midstate.  Scripts are
 * addressed as the messages of the *_lens calls: script i at script + i * stride_bytes, min(lens[i], stride_bytes) bytes of it, or script_bytes (< 2^32) with
 * lens = NULL.  leaf_version: n x u8 of device memory, or NULL for leaf_version_all (<= 255) on every lane.  The compact size is 1, 3 or 5 bytes (< 0xfd; <= 0xffff:
 * fd and u16 little-endian; else fe and u32 little-endian); the 2 to 6 prefix bytes are built in registers and the script follows them shifted against the word
 * grid: nothing is staged in memory, and no byte at or behind a script is loaded.
 *
 * taproot_merkle_path: lane i starts with k = leaf[i] and, for j < depth, takes node e_j = the 32 bytes at path + i * path_stride_bytes + 32 j, in the order a
 * control block holds them, to k = SHA256(tag || tag || min(k, e_j) || max(k, e_j)), tag = SHA256("TapBranch") -- the order is that of the 32 bytes, the
 * integers'.  root[i] = the final k; depth 0 gives the leaf (path may then be NULL).  depth: n x u8, or NULL for depth_all.  A depth above 128 (BIP-341's bound)
 * gives ok[i] = 0 and root = 0, else ok[i] = 1.  Two compressions a step, the second a constant padding block; the loop runs per lane.  Any alignment of path
 * (word loads where base and stride are multiples of 4).  root must not alias leaf. */
int ecsimd_hip_tapleaf_hash(ecsimd_hip_ctx*, const uint8_t* script, size_t script_bytes, size_t stride_bytes, const uint32_t* lens, const uint8_t* leaf_version,
                            uint32_t leaf_version_all, uint64_t* e, size_t n);
int ecsimd_hip_taproot_merkle_path(ecsimd_hip_ctx*, const uint64_t* leaf, const uint8_t* path, size_t path_stride_bytes, const uint8_t* depth, uint32_t depth_all,
                                   uint64_t* root, uint8_t* ok, size_t n);
/* HASH160 of the SEC1 encoding of n public keys (qx, qy), 4 x u64 limbs each: compressed != 0: (02 | parity of qy) || be32(qx), 33 bytes, one SHA-256 and one
 * RIPEMD-160 compression; compressed == 0: 04 || be32(qx) || be32(qy), 65 bytes, two and one.  The encoding is built in registers and never reaches memory.  No
 * validation: the call hashes the encoding of the integers it is given ((0, 0) hashes as 02 || 32 zero bytes does).  out20 as above.  PUBLIC data.
 * Stream-ordered; no workspace.  (The hash of a SECRET key d's public key: ecsimd_hip_scalar_mult_base with ECSIMD_HIP_ALG_WINDOWED |
 * ECSIMD_HIP_ALG_CONSTANT_TIME | ECSIMD_HIP_OUT_AFFINE, then this call on the public result.) */
int ecsimd_hip_btc_pubkey_hash(ecsimd_hip_ctx*, const uint64_t* qx, const uint64_t* qy, uint8_t* out20, size_t n, int compressed);
/* BIP-341 Taproot key tweaks.  secp256k1 only: no curve id.  Keys, tweaks and merkle roots are 4 x u64 little-endian limbs per element (the integer whose 32
 * big-endian bytes the BIP writes), 16-byte aligned.  Stream-ordered, nothing is read back.  No ECSIMD_HIP_REF_SQUARE_COMPAT form (ERR_BAD_ARG on a context with
 * that option).  Any n (2^22 at a time).
 *
 * xonly_tweak_add, PUBLIC data: Q = P + t G with P = the even-y point of x coordinate px.  ok[i] = 1 iff px < p and lifts, t < n and Q is finite; then
 * qx = x(Q) and parity = y(Q) & 1, else qx = 0 and parity = 0.  t = 0 is valid and gives Q = P: qx = px, parity = 0.  t G = P (a doubling) is handled; t G = -P
 * gives ok = 0.  Per chunk: one kernel lifts and range-checks, t G comes from the public comb (indexed by the digits of t: not for secrets -- the 20-bit table in
 * device memory once it exists or n >= 2^16, else the signed 7-bit table in LDS), one kernel adds, ONE simultaneous inversion, one kernel accepts.  qx must not
 * alias an input.  Workspace: 193 B per element of a chunk.
 *
 * taproot_tweak_pubkey, PUBLIC data: the same with t = int(SHA256(tag || tag || be32(px) || h)), tag = SHA256("TapTweak"), made in the first kernel from the tag
 * block's midstate.  merkle_root = NULL (the call's, not the lane's): key-path-only spending, no h: 32 bytes of data, one compression; otherwise h = merkle_root[i],
 * two compressions.  t is NOT reduced modulo n: t >= n gives ok = 0 (probability ~2^-128).  The hash cannot be 0 in practice; if it were, the lane would return
 * what xonly_tweak_add returns for t = 0: ok = 1, qx = px, parity = 0.  The caller checks a control block by comparing qx and parity (ecsimd_hip_cmp_eq).
 * Workspace as above.
 *
 * taproot_tweak_seckey, SECRET data: d_out = d' + t mod n with d' = d where y(d G) is even, n - d where it is odd, and t as above from x(d G) -- the secret key of
 * the output key Q, ready for ecsimd_hip_schnorr_sign.  px (optional output, may be NULL) = x(d G), the internal x-only key.  ok[i] = 0 and d_out = px = 0 where d
 * is not in [1, n - 1], t >= n, or the sum is 0 (t = 0 would give d_out = d').  d, d', d_out, the Jacobian and the affine d G are SECRETS until returned, and so is
 * t while px is: d G runs on the constant-time comb (the kernel of ALG_WINDOWED | ALG_CONSTANT_TIME) and the select-only simultaneous inversion, the kernel behind
 * them selects by masks -- no branch, address or lane mask in force at a memory access depends on a secret and no bit is declassified (tools/ct_check.py
 * check_secret_flow on the shipped ISA: tests/test_btc_cpu.py).  merkle_root is public but treated no differently.  Every workspace byte the call used is zeroed
 * on the stream before it returns, whatever the launches said.  d_out and px must not alias an input or each other.  Workspace: 160 B per element of a chunk. */
int ecsimd_hip_xonly_tweak_add(ecsimd_hip_ctx*, const uint64_t* px, const uint64_t* t, uint64_t* qx, uint8_t* parity, uint8_t* ok, size_t n);
int ecsimd_hip_taproot_tweak_pubkey(ecsimd_hip_ctx*, const uint64_t* px, const uint64_t* merkle_root, uint64_t* qx, uint8_t* parity, uint8_t* ok, size_t n);
int ecsimd_hip_taproot_tweak_seckey(ecsimd_hip_ctx*, const uint64_t* d, const uint64_t* merkle_root, uint64_t* d_out, uint64_t* px, uint8_t* ok, size_t n);
/* SHA-512 and HMAC-SHA-512 (RFC 2104) over n equal-length messages, message i at msg + i * stride_bytes, msg_bytes long, as for ecsimd_hip_sha256: any length
 * including 0 (msg may then be NULL), stride_bytes >= msg_bytes, any alignment (word loads where base and stride are multiples of 4, byte loads otherwise).
 * PUBLIC data: the loads and the block loop follow the length; do not hash a secret with these.  out64: n x 64 bytes of device memory, 16-byte aligned: lane
 * i's digest at out64 + 64 i, its bytes in order.  Stream-ordered; no workspace.  One message per lane; the eight 64-bit state words and the sixteen-word
 * schedule stay in registers, the 80 rounds are unrolled.
 *   sha512        SHA-512(m): c compressions for a message of c 128-byte blocks (padding and the 128-bit length included).
 *   hmac_sha512   HMAC(key, m).  Lane i's key: key_bytes bytes at key + i * key_stride_bytes; key_stride_bytes == 0: ONE key for the whole call (otherwise
 *                 key_stride_bytes >= key_bytes).  A key of at most 128 bytes is zero-padded to one block, a longer one is hashed first.  The key's ipad and
 *                 opad blocks are compressed once each, the message is absorbed behind the first, ONE outer block finishes: c + 3 compressions. */
int ecsimd_hip_sha512(ecsimd_hip_ctx*, const uint8_t* msg, size_t msg_bytes, size_t stride_bytes, uint8_t* out64, size_t n);
int ecsimd_hip_hmac_sha512(ecsimd_hip_ctx*, const uint8_t* key, size_t key_bytes, size_t key_stride_bytes,
                           const uint8_t* msg, size_t msg_bytes, size_t stride_bytes, uint8_t* out64, size_t n);
/* BIP-32 hierarchical key derivation.  secp256k1 only: no curve id.  Keys and chain codes are 4 x u64 little-endian limbs per element (the integer whose 32
 * big-endian bytes the BIP writes), 16-byte aligned.  index: n x u32 of device memory, 4-byte aligned, one index per lane; index == NULL: every lane uses
 * index_all.  An index is PUBLIC; i >= 2^31 is a hardened one.  Stream-ordered, nothing is read back.  No ECSIMD_HIP_REF_SQUARE_COMPAT form (ERR_BAD_ARG on a
 * context with that option).  Any n (2^22 at a time); outputs must not alias inputs or each other.  Depth, parent fingerprint (the first four bytes of
 * ecsimd_hip_btc_pubkey_hash) and the Base58Check strings are the caller's bookkeeping.
 * Three refusals exist that no test can reach -- IL >= n, a child key of 0, an infinite child point: each has probability about 2^-128 and an input that
 * provokes one would have to invert HMAC-SHA-512.
 *
 * bip32_master, SECRET data: I = HMAC-SHA512("Bitcoin seed", seed), k = IL, c = IR.  Lane i's seed: seed_bytes bytes (16 .. 64, the same for every lane, else
 * ERR_BAD_ARG) at seed + i * stride_bytes, any alignment.  The key's two midstates are compile-time constants: two compressions per lane.  ok[i] = 0 and
 * k = c = 0 where IL = 0 or IL >= n.  Masks and selects only; only the public length steers the loads.  No workspace.
 *
 * bip32_ckd_priv, SECRET data: I = HMAC-SHA512(c_par, 00 || ser256(k_par) || ser32(i)) for a hardened i, HMAC-SHA512(c_par, serP(k_par G) || ser32(i))
 * otherwise; k_child = IL + k_par mod n, c_child = IR.  ok[i] = 0 and k_child = c_child = 0 where k_par is not in [1, n - 1], IL >= n or k_child = 0.  k_par,
 * c_par, the Jacobian and the affine k_par G, I, k_child and c_child are SECRETS: k_par G runs on the constant-time comb (the kernel of ALG_WINDOWED |
 * ALG_CONSTANT_TIME) and the select-only simultaneous inversion, the kernel behind them builds the 37 bytes in registers, chooses between the two forms by a
 * select on bit 31 of the index and selects by masks -- no branch, address or lane mask in force at a memory access depends on a secret and no bit is
 * declassified (tools/ct_check.py check_secret_flow on the shipped ISA: tests/test_bip32_cpu.py).  Four compressions per lane.
 * flags = ECSIMD_HIP_BIP32_ALL_HARDENED: the caller's promise that every index has bit 31 set; the comb and the inversion are skipped and no workspace is used.  A
 * lane that breaks the promise returns ok = 0 and zeros.  With index == NULL the call sees index_all and takes that route by itself.  Every workspace byte the
 * call used is zeroed on the stream before it returns, whatever the launches said.  Workspace: 160 B per element of a chunk, none on the hardened-only route.
 *
 * bip32_ckd_pub, PUBLIC data: I = HMAC-SHA512(c_par, serP(K) || ser32(i)) with K = (qx, qy); (cx, cy) = IL G + K, c_child = IR.  ok[i] = 1 iff i < 2^31, K is
 * on the curve (qx, qy < p), IL < n and the sum is finite; else cx = cy = c_child = 0.  Per chunk: one kernel hashes and validates, IL G comes from the public
 * comb (indexed by the digits of IL: not for secrets), k_tweak_add adds, ONE simultaneous inversion, one kernel accepts -- the chain of
 * ecsimd_hip_xonly_tweak_add, keeping both coordinates.  Workspace: 193 B per element of a chunk. */
enum { ECSIMD_HIP_BIP32_ALL_HARDENED = 1 };
int ecsimd_hip_bip32_master(ecsimd_hip_ctx*, const uint8_t* seed, size_t seed_bytes, size_t stride_bytes,
                            uint64_t* k, uint64_t* c, uint8_t* ok, size_t n);
int ecsimd_hip_bip32_ckd_priv(ecsimd_hip_ctx*, const uint64_t* k_par, const uint64_t* c_par, const uint32_t* index, uint32_t index_all,
                              uint64_t* k_child, uint64_t* c_child, uint8_t* ok, size_t n, int flags);
int ecsimd_hip_bip32_ckd_pub(ecsimd_hip_ctx*, const uint64_t* qx, const uint64_t* qy, const uint64_t* c_par, const uint32_t* index, uint32_t index_all,
                             uint64_t* cx, uint64_t* cy, uint64_t* c_child, uint8_t* ok, size_t n);
/* PBKDF2 (RFC 8018 section 5.2) with HMAC-SHA-512 as the PRF over n (password, salt) pairs, one per lane, and BIP-39's seed, which is one such derivation.
 * Lane i's password: pw + i * pw_stride_bytes, its salt: salt + i * salt_stride_bytes (device memory).  pw_lens / salt_lens as lens of ecsimd_hip_keccak256: NULL:
 * every lane uses pw_bytes / salt_bytes (stride >= bytes); otherwise n x u32 of device memory, 4-byte aligned, lane i uses lens[i] <= stride bytes (a larger value
 * is read as the stride), the stride is at most 2^30 and pw_bytes / salt_bytes is ignored.  Without lens, pw_bytes and salt_bytes are at most 2^30.  salt_stride_bytes == 0: ONE salt of salt_bytes bytes for the whole call, as the key of
 * ecsimd_hip_hmac_sha512; salt_lens must then be NULL.  Any length including 0 (the pointer may then be NULL), any alignment (word loads where base and stride are
 * multiples of 4, byte loads otherwise).  A password of at most 128 bytes is zero-padded to the key block, a longer one is hashed first.  iterations >= 1,
 * 1 <= dk_bytes <= 2^30, out_stride_bytes >= dk_bytes: lane i's derived key at out + i * out_stride_bytes, its bytes in order, the bytes between two keys untouched; out
 * must not alias an input.  Anything else: ERR_BAD_ARG.  n = 0 succeeds.  ECSIMD_HIP_REF_SQUARE_COMPAT does not concern this call (no curve arithmetic): accepted.
 * SECRET: the passwords' and the salts' bytes, the HMAC midstates, every U and T and the derived key.  PUBLIC: the lengths, iterations and dk_bytes: they steer the
 * loads and the block loops (per lane where lens is given), as seed_bytes does in ecsimd_hip_bip32_master.  No branch, address or lane mask in force at a memory
 * access depends on a secret and no bit is declassified (tools/ct_check.py check_secret_flow on the shipped ISA: tests/test_bip39_cpu.py).
 * Cost: 2 (iterations - 1) + 4 or so SHA-512 compressions per lane and 64-byte output block; the blocks of a long key run side by side (the grid's second
 * dimension).  A launch runs at most ECSIMD_HIP_PBKDF2_SLICE iterations over a bounded number of lanes, so that no launch holds a shared
 * device for long whatever the caller's count.  iterations <= ECSIMD_HIP_PBKDF2_SLICE: one launch per chunk of lanes and no workspace.  Beyond: the lane's two
 * midstates, U and T lie in the context workspace between launches, 256 B per lane and block of a chunk, and every byte used is zeroed on the stream before the call
 * returns, whatever the launches said.  Stream-ordered, nothing is read back.  Any n.
 *
 * bip39_seed: seed64[64 i ..] = PBKDF2-HMAC-SHA512(password = mnemonic i, salt = "mnemonic" || passphrase i, 2048 iterations, 64 bytes): one launch per chunk, no
 * workspace; the eight bytes of the prefix reach the kernel by value, no salt is staged.  mnemonic / passphrase as pw / salt above (passphrase_stride_bytes == 0: one
 * passphrase for the call; passphrase == NULL with passphrase_bytes == 0: the empty passphrase).  The sentence and the passphrase are taken as BYTES: Unicode
 * normalisation (NFKD), the word list and the checksum are the caller's -- a sentence that BIP-39 would reject derives a seed like any other.  The seed is the
 * `seed` of ecsimd_hip_bip32_master (seed_bytes = stride_bytes = 64). */
enum { ECSIMD_HIP_PBKDF2_SLICE = 4096 };
int ecsimd_hip_pbkdf2_hmac_sha512(ecsimd_hip_ctx*, const uint8_t* pw, size_t pw_bytes, size_t pw_stride_bytes, const uint32_t* pw_lens,
                                  const uint8_t* salt, size_t salt_bytes, size_t salt_stride_bytes, const uint32_t* salt_lens,
                                  uint32_t iterations, uint8_t* out, size_t dk_bytes, size_t out_stride_bytes, size_t n);
int ecsimd_hip_bip39_seed(ecsimd_hip_ctx*, const uint8_t* mnemonic, size_t mnemonic_bytes, size_t mnemonic_stride_bytes, const uint32_t* mnemonic_lens,
                          const uint8_t* passphrase, size_t passphrase_bytes, size_t passphrase_stride_bytes, const uint32_t* passphrase_lens,
                          uint8_t* seed64, size_t n);
/* Diagnostic (r5): ONE function of the reduced-radix layer the multiplication-bound loops run on (fe29.cuh: nine signed 29-bit limbs in 32-bit words,
 * Montgomery radix 2^261, lazy carries) on RAW operands -- int32 limbs exactly as a loop holds them between two operations: element e's coordinate c, limb l at
 * in[(e * NIN + c) * 9 + l] (device memory).  What tests use to hand the device the states and operand pairs at which the interval proofs of
 * tools/radix29_model.py reach their largest 64-bit columns (tests/golden/fe29_witnesses.json) and compare the result limb for limb with the exact model; no
 * other entry point can produce such inputs (their operands enter the loops as tight limbs).  op (NIN -> NOUT coordinates):
 *   0 zdau29 (x1, x2, dx, y1, dy, z -> the same six; swap != 0 exchanges the two output points)      1 madd29 (X, Y, Z, x2, y2 -> X, Y, Z)      2 jdbl29 (X, Y, Z ->)
 *   3 dbl_add29 (X, Y, Z, x2, y2 ->)    4 madd29_hr + madd29v_finish    5 pdbl29, 6 padd29 (secp256k1: the complete law)    7 mul29 (a, b -> r)    8 sqr29 (a -> r)
 *   9 gjdbl29 (X, Y, Z, W = a Z^4 -> the same four; swap != 0: the doubled point's W is formed)    10 zaddu29 (x1, y1, x2, y2, z -> rx, ry, x1', y1', z', dx)
 * curve: 0 / 1 (for secp256k1 the loops' own domain: values x * 2^261 of the CLASSICAL x; ops 0-8, secp256k1 also 10), or a registered curve id (ops 0, 1, 3, 7, 8, 9,
 * 10: the dense reduction; the window loop of k_gvarwin.hip).
 * Operands outside the proven bounds give whatever 32- / 64-bit wrap-around gives. */
int ecsimd_hip_fe29_raw(ecsimd_hip_ctx* ctx, int curve, int op, const int32_t* in, int32_t* out, size_t n, int swap);
/* Diagnostic: the context's grow-only scratch block (device pointer and size; NULL / 0 before the first call that needed one).  What a test reads
 * back to see that ecdsa_sign left no nonce-derived data behind (tests/test_gpu_fields.py); valid until the next call that grows the block. */
int ecsimd_hip_workspace_info(ecsimd_hip_ctx* ctx, const void** dptr, size_t* bytes);
/* scalar_mult with every array in HOST memory (n elements each; pageable is fine): the PCIe-inclusive form of the hot path.  Same curve ids, flags and
 * meaning as ecsimd_hip_scalar_mult (x = y = NULL with ECSIMD_HIP_BASE_GENERATOR: k G; OUT_AFFINE: oz unused, oy optional).  Chunks of 2^19 elements
 * alternate between the context and a helper context it creates on first use (a second stream): the copies of one chunk overlap the ladder of its
 * neighbour.  Synchronous -- returns with the results in place; refuses under stream capture.  One MI355X, 2^22 elements of pageable memory: 56 M scalar mults/s against
 * 58 with the arrays resident in HBM (reuse the output arrays: fresh pages are first touched inside the call).  The reference's own types instead of arrays: integration/scalar_mult_p256_adapter.cpp. */
int ecsimd_hip_scalar_mult_host(ecsimd_hip_ctx*, int curve, const uint64_t* k, const uint64_t* x, const uint64_t* y,
                                uint64_t* ox, uint64_t* oy, uint64_t* oz, size_t n, int flags);
/* lib/scalar_mult_p256.cpp:10-12: scalar_mult_p256(x, P) -- P-256, base in Montgomery form with
 * Z = mgry(1), Jacobian Montgomery output. */
int ecsimd_hip_scalar_mult_p256(ecsimd_hip_ctx*, const uint64_t* k, const uint64_t* xm, const uint64_t* ym,
                                uint64_t* ox, uint64_t* oy, uint64_t* oz, size_t n);

/* ---- synthetic inputs and measurement (bench / tests) --------------------------------- */
/* word w of element i of stream s = splitmix64(seed ^ (s << 56) ^ (4 i + w));
 * clear_top_bits > 0 clears that many top bits of limb 3 (field elements < 2^255 < p). */
int ecsimd_hip_fill_random(ecsimd_hip_ctx*, uint64_t* out, size_t n, uint64_t seed, uint64_t stream, uint64_t first_index, int clear_top_bits);
/* Dependency-free v_mad_u64_u32 stream: the integer-multiply roofline denominator.  Returns the
 * number of mad32 executed in *mads; elapsed device time in *ms (HIP events on the ctx stream, waited for: refuses under stream capture). */
int ecsimd_hip_peak_mad32(ecsimd_hip_ctx*, int iters, double* mads, double* ms);

/* ---- device groups: one batch over several GPUs -------------------------------
 * The reference is single-threaded and has no collectives (nothing to cite); BASELINE.json north_star asks for
 * batches sharded across the GPUs of a node "with RCCL over xGMI only for the final gather", host code behind this ABI.
 * A group owns one context per listed device.  Member m of G owns the contiguous slice shard_range(n, m, G) of a
 * batch (the first n % G members take one element more); no collective touches the data path; the result shards
 * are gathered to member 0's device memory by one grouped ncclSend / ncclRecv exchange on a second stream of member 0's
 * device, so that member 0's next ladder overlaps it.  RCCL is looked up at run time when the group has more than one
 * device -- the copy the process already has (soname librccl.so.1, e.g. torch's) if there is one, else ROCm's; the library
 * needs RCCL neither to build nor to link.  A device may be listed twice, in which case those members exchange
 * by device copies (how a one-GPU machine exercises the bookkeeping).  One host thread drives a group; every group
 * entry point leaves the caller's current HIP device as it found it (the per-context entry points above select their
 * context's device and leave it selected).
 *
 * EXPERIMENTAL until a machine with two or more GPUs has run tests/test_gpu_parity.py::test_device_group_behind_the_c_abi
 * with distinct devices: the bookkeeping, staging, offsets and the device-copy gather run in every GPU test run, RCCL is
 * loaded and exercised on a one-rank communicator (ecsimd_hip_group_rccl_selftest), but the ncclCommInitAll +
 * multi-device ncclSend / ncclRecv exchange itself has only been checked against RCCL's documented contract. */
typedef struct ecsimd_hip_group ecsimd_hip_group;
enum {
  ECSIMD_HIP_GROUP_NO_GATHER = 0x10000   /* ecsimd_hip_group_scalar_mult only: compute, leave every shard where its member wrote it
                                            (member 0: its slice of ox/oy/oz; the others: group staging).  For timing the ladders
                                            without the exchange ("throughput with and without the gather") */
};
int ecsimd_hip_shard_range(size_t n_total, int member, int members, size_t* first, size_t* count);   /* pure host arithmetic */
int ecsimd_hip_group_init(const int* devices, int n_devices, ecsimd_hip_group** group);
int ecsimd_hip_group_destroy(ecsimd_hip_group* group);
int ecsimd_hip_group_size(const ecsimd_hip_group* group);
int ecsimd_hip_group_uses_rccl(const ecsimd_hip_group* group);                 /* 1 when the gather goes through RCCL */
int ecsimd_hip_group_rccl_version(const ecsimd_hip_group* group);              /* ncclGetVersion of that RCCL (22606 = 2.26.6); 0 without RCCL */
ecsimd_hip_ctx* ecsimd_hip_group_context(ecsimd_hip_group* group, int member); /* e.g. to allocate on that device, set options */
const char* ecsimd_hip_group_last_error(const ecsimd_hip_group* group);
/* curve_group.h:189-218 over the group, device-resident: k[m], x[m], y[m] = member m's slice in ITS device memory;
 * ox, oy, oz = n elements each in member 0's device memory; flags as ecsimd_hip_scalar_mult (| GROUP_NO_GATHER): with
 * OUT_AFFINE oz may be NULL, and oy too (x only: P-256 then runs the ladder without Z on every member).
 * Asynchronous -- except that a call which has to grow a member's staging block (the first one, or a larger batch than
 * any before) drains that member's stream and the gather stream first.  Calls may follow one another without a sync:
 * a member's next ladder is ordered behind the exchange that reads its staging.  ecsimd_hip_group_sync waits for every
 * member and the gather stream and reports how long the last gather took (milliseconds; NULL to skip; -1 if there was none). */
int ecsimd_hip_group_scalar_mult(ecsimd_hip_group* group, int curve, const uint64_t* const* k, const uint64_t* const* x, const uint64_t* const* y,
                                 uint64_t* ox, uint64_t* oy, uint64_t* oz, size_t n, int flags);
int ecsimd_hip_group_sync(ecsimd_hip_group* group, double* last_gather_ms);
/* Device time (ms, HIP events on that member's stream) of member `member`'s LAST ladder launch; call after group_sync.
 * -1 if the member has not launched anything. */
int ecsimd_hip_group_member_ms(ecsimd_hip_group* group, int member, double* ms);
/* What one GPU can verify of the RCCL side: loads RCCL as group_init does, creates a one-rank communicator on member 0's
 * device and moves `elements` 256-bit elements between two buffers with the calls the gather uses (grouped ncclSend /
 * ncclRecv of ncclUint64, the gather stream).  0 = the bytes arrived intact. */
int ecsimd_hip_group_rccl_selftest(ecsimd_hip_group* group, size_t elements);
/* The same with every array in HOST memory (n elements each): slices copied in, computed, gathered, copied out.
 * Synchronous, and a CONVENIENCE path: the arrays are pageable as far as the library knows, so the runtime stages the
 * copies and they do not overlap the ladders (1.5 GB each way at BASELINE config 4).  Callers that want the overlap keep
 * pinned buffers, device-resident shards and the device form above. */
int ecsimd_hip_group_scalar_mult_host(ecsimd_hip_group* group, int curve, const uint64_t* k, const uint64_t* x, const uint64_t* y,
                                      uint64_t* ox, uint64_t* oy, uint64_t* oz, size_t n, int flags);

#ifdef __cplusplus
}
#endif
#endif /* ECSIMD_HIP_H */
