// capi.hip -- the C ABI of include/ecsimd_hip.h: argument checks, context/stream handling and
// dispatch to the kernel launchers of kernels.h (gfx950 only; no CPU fallback of any kind).
//
// One field element / one curve point per lane, 256-thread workgroups.  The path is integer-VALU
// bound by three orders of magnitude (~2900 multiplies per byte moved), so there is
// no LDS staging, no XCD-aware remap and no MFMA: workgroups never share data and HBM sees ~0.1 %
// of its bandwidth.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <initializer_list>
#include <mutex>
#include <new>
#include <vector>

#include "../../include/ecsimd_hip.h"
#include "../../include/ecsimd_ed25519.h"
#include "../../include/ecsimd_x25519.h"
#include "../../include/ecsimd_p384.h"
#include "../../include/ecsimd_bls12_381.h"
#include "../../include/ecsimd_bls12_381_g2.h"
#include "../../include/ecsimd_sm2.h"
#include "../../include/ecsimd_msm.h"
#include "../../include/ecsimd_schnorr_batch.h"
#include "../../include/ecsimd_ed25519_batch.h"
#include "../../include/ecsimd_ntt.h"
#include "kernels.h"
#include "point.cuh"   // curve constants for ecsimd_hip_get_constant (host-side constexpr use only)
#include "gfield.cuh"  // gmod: a run-time modulus as the generic field kernels take it
#include "gcurve.cuh"  // gcurve: a run-time curve as the generic point kernels and the ladder take it
#include "ntt.cuh"     // the transform's schedule, one pass's geometry and the portable field the domain tables are built with

using namespace ecsimd_hip;
using launch::BLOCK;

namespace {
// Stream-ordered store of a 256-bit kernel argument into device memory (the shared scalar of
// scalar_mult_1s): no host buffer has to outlive the call.
__global__ void k_store_words(launch::words8 w, uint32_t* dst) {
  if (threadIdx.x < 8) dst[threadIdx.x] = w.w[threadIdx.x];
}
void store_words(hipStream_t s, const launch::words8& w, uint32_t* dst) {
  hipLaunchKernelGGL(k_store_words, dim3(1), dim3(64), 0, s, w, dst);
}
}  // namespace

// curve dispatch for the per-curve translation units
namespace ecsimd_hip { namespace launch {
// DISPATCH: the kernels every instance has (k_point.inc, k_ladder.inc) -- the two API curves and their
// ECSIMD_HIP_REF_SQUARE_COMPAT twins; DISPATCH2: the kernels of the other algorithms (k_affine.inc, k_varwin.inc), API curves only.
#define DISPATCH(fn, ...) do { switch (curve) { case CURVE_P256: point_launch<CURVE_P256>::fn(__VA_ARGS__); break; case CURVE_SECP256K1: point_launch<CURVE_SECP256K1>::fn(__VA_ARGS__); break; \
    case CURVE_P256_REFSQR: point_launch<CURVE_P256_REFSQR>::fn(__VA_ARGS__); break; default: point_launch<CURVE_SECP256K1_REFSQR>::fn(__VA_ARGS__); break; } } while (0)
#define DISPATCH2(fn, ...) do { if (curve == CURVE_P256) point_launch<CURVE_P256>::fn(__VA_ARGS__); else point_launch<CURVE_SECP256K1>::fn(__VA_ARGS__); } while (0)
void from_affine(hipStream_t s, int curve, const uint64_t* x, const uint64_t* y, uint64_t* jx, uint64_t* jy, uint64_t* jz, size_t n) { DISPATCH(from_affine, s, x, y, jx, jy, jz, n); }
void to_affine(hipStream_t s, int curve, const uint64_t* jx, const uint64_t* jy, const uint64_t* jz, uint64_t* x, uint64_t* y, size_t n) { DISPATCH(to_affine, s, jx, jy, jz, x, y, n); }
void compute_y(hipStream_t s, int curve, const uint64_t* x, uint64_t* y, uint8_t* ok, size_t n) { DISPATCH(compute_y, s, x, y, ok, n); }
void dblu(hipStream_t s, int curve, uint64_t* px, uint64_t* py, uint64_t* pz, uint64_t* rx, uint64_t* ry, uint64_t* rz, size_t n) { DISPATCH(dblu, s, px, py, pz, rx, ry, rz, n); }
void zaddu(hipStream_t s, int curve, uint64_t* px, uint64_t* py, uint64_t* pz, const uint64_t* qx, const uint64_t* qy, uint64_t* rx, uint64_t* ry, uint64_t* rz, size_t n) { DISPATCH(zaddu, s, px, py, pz, qx, qy, rx, ry, rz, n); }
void zdau(hipStream_t s, int curve, const uint64_t* px, const uint64_t* py, const uint64_t* pz, uint64_t* qx, uint64_t* qy, uint64_t* qz, uint64_t* rx, uint64_t* ry, uint64_t* rz, size_t n) { DISPATCH(zdau, s, px, py, pz, qx, qy, qz, rx, ry, rz, n); }
void add_z2_1(hipStream_t s, int curve, const uint64_t* ax, const uint64_t* ay, const uint64_t* az, const uint64_t* bx, const uint64_t* by, uint64_t* rx, uint64_t* ry, uint64_t* rz, size_t n) { DISPATCH(add_z2_1, s, ax, ay, az, bx, by, rx, ry, rz, n); }
void trplu(hipStream_t s, int curve, uint64_t* px, uint64_t* py, uint64_t* pz, uint64_t* rx, uint64_t* ry, uint64_t* rz, size_t n) { DISPATCH(trplu, s, px, py, pz, rx, ry, rz, n); }
void scalar_mult(hipStream_t s, int curve, const uint64_t* k, int k_stride, const uint64_t* x, const uint64_t* y, uint64_t* ox, uint64_t* oy, uint64_t* oz, size_t n, int flags) { DISPATCH(scalar_mult, s, k, k_stride, x, y, ox, oy, oz, n, flags); }
void zdau_repeat(hipStream_t s, int curve, const uint64_t* px, const uint64_t* py, const uint64_t* pz, const uint64_t* qx, const uint64_t* qy, uint64_t* rx, uint64_t* ry, uint64_t* sx, uint64_t* sy, uint64_t* oz, size_t n, int iters, uint64_t swap_bits, int radix) { DISPATCH(zdau_repeat, s, px, py, pz, qx, qy, rx, ry, sx, sy, oz, n, iters, swap_bits, radix); }
void to_affine_batched(hipStream_t s, int curve, const uint64_t* jx, const uint64_t* jy, const uint64_t* jz, uint64_t* x, uint64_t* y, size_t n, bool in_fast) { DISPATCH2(to_affine_batched, s, jx, jy, jz, x, y, n, in_fast); }
void pack_table(hipStream_t s, int curve, const uint64_t* tx, const uint64_t* ty, uint32_t* table) { DISPATCH2(pack_table, s, tx, ty, table); }
void pack_table_signed(hipStream_t s, int curve, int wbits, const uint64_t* tx, const uint64_t* ty, uint32_t* table) { DISPATCH2(pack_table_signed, s, wbits, tx, ty, table); }
void base_windowed_signed(hipStream_t s, int curve, const uint64_t* k, const uint32_t* table, uint64_t* ox, uint64_t* oy, uint64_t* oz, size_t n, bool constant_time) { DISPATCH2(base_windowed_signed, s, k, table, ox, oy, oz, n, constant_time); }
void inverse_batched(hipStream_t s, int curve, const uint64_t* a, uint64_t* out, size_t n) { DISPATCH2(inverse_batched, s, a, out, n); }
void x_mod_n_equals(hipStream_t s, int curve, const uint64_t* x, const uint8_t* finite, const uint64_t* r, uint8_t* ok, size_t n) { DISPATCH2(x_mod_n_equals, s, x, finite, r, ok, n); }
void affine_add_batched(hipStream_t s, int curve, const uint64_t* ax, const uint64_t* ay, const uint64_t* bx, const uint64_t* by, uint64_t* rx, uint64_t* ry, uint8_t* finite, size_t n) { DISPATCH2(affine_add_batched, s, ax, ay, bx, by, rx, ry, finite, n); }
void base_windowed(hipStream_t s, int curve, const uint64_t* k, const uint32_t* table, uint64_t* ox, uint64_t* oy, uint64_t* oz, size_t n, bool constant_time) { DISPATCH2(base_windowed, s, k, table, ox, oy, oz, n, constant_time); }
void pack_table_big(hipStream_t s, int curve, const uint64_t* tx, const uint64_t* ty, uint32_t* table) { DISPATCH2(pack_table_big, s, tx, ty, table); }
void base_windowed_big(hipStream_t s, int curve, const uint64_t* k, const uint32_t* table, uint64_t* ox, uint64_t* oy, uint64_t* oz, size_t n) { DISPATCH2(base_windowed_big, s, k, table, ox, oy, oz, n); }
void add_mixed_complete(hipStream_t s, int curve, const uint64_t* ax, const uint64_t* ay, const uint64_t* az, const uint64_t* bx, const uint64_t* by, uint64_t* rx, uint64_t* ry, uint64_t* rz, size_t n) { DISPATCH2(add_mixed_complete, s, ax, ay, az, bx, by, rx, ry, rz, n); }
void varwin_scalar_mult(hipStream_t s, int curve, const uint64_t* k, int k_stride, const uint64_t* x, const uint64_t* y, int flags, uint64_t* scratch, uint64_t* ox, uint64_t* oy, size_t n) { DISPATCH2(varwin_scalar_mult, s, k, k_stride, x, y, flags, scratch, ox, oy, n); }
#undef DISPATCH
#undef DISPATCH2
} }

// ================================================================== host side
struct ecsimd_hip_ctx {
  int device;
  hipStream_t own_stream;
  hipStream_t stream;
  hipEvent_t handoff;  // orders a newly selected stream after the work already enqueued on the previous one
  int cus;
  uint32_t* sink;      // 4 KiB scratch: peak-probe sink [0, 1024) and the shared scalar at word 1024-8
  uint32_t* window_table[2];   // per curve: 64 x 8 affine odd multiples (2d + 1) 16^w G (built on first use)
  uint32_t* windowct_table[2]; // per curve: the 5-bit odd-digit table of the constant-time comb (CT_WBITS)
  uint32_t* window6_table[2];  // per curve: signed-window table (SIGNED_WBITS bits): (2d + 1) 2^(WB i) G, d = 0..2^(WB-1) - 1
  uint32_t* window16_table[2]; // per curve: signed BIG_WINDOW_BITS-bit windows in device memory (20 bits: 13 x 524 288 entries, 436 MB)
  uint64_t* workspace;         // grow-only scratch for the windowed path's Jacobian intermediates
  size_t workspace_bytes;
  uint64_t* base_special[2];   // per curve: the reference ladder's 3 degenerate scalars and its affine results for them on G (small-batch route of scalar_mult_base)
  uint8_t* valid;              // grow-only: per-lane public-key validity of double_scalar_mult / ecdsa_verify_rx
  size_t valid_bytes;
  int ref_square;              // ecsimd_hip_set_ref_square_compat: the reference's square() as written (mul.h:160-212)
  struct gcomb_entry { int curve; uint32_t* table; uint64_t* special; uint32_t* table7; uint32_t* table5; uint32_t* table20; };      // table7: the signed 7-bit comb (ALG_WINDOWED_SIGNED); table5: the constant-time 5-bit comb; table20: the 20-bit comb in device memory (ALG_WINDOWED_BIG, 436 MB)
  std::vector<gcomb_entry> gcomb;   // per registered curve: the 4-bit odd-digit table of multiples of its generator (k_gcomb.hip) and, for the small-batch route, the ladder's
                                    // three degenerate scalars with its affine results for them on G (as base_special); built on first use
  ecsimd_hip_ctx* helper;      // ecsimd_hip_scalar_mult_host: the second stream's context (created on first use, destroyed with this one)
  uint64_t* hstage; size_t hstage_bytes;    // ... and this context's staging block for one chunk (grow-only)
  uint64_t* pinned; size_t pinned_bytes;    // btc_merkle_root: the pinned host block its node offsets are uploaded from (grow-only) ...
  hipEvent_t pinned_copied;                 // ... and the event behind the last upload: the next one waits for it before it overwrites the block
  char err[256];
};

namespace {

int fail(ecsimd_hip_ctx* ctx, hipError_t e, const char* what) {
  if (ctx) snprintf(ctx->err, sizeof ctx->err, "%s: %s", what, hipGetErrorString(e));
  return ECSIMD_HIP_ERR_HIP;
}
int bad(ecsimd_hip_ctx* ctx, const char* what) {
  if (ctx) snprintf(ctx->err, sizeof ctx->err, "bad argument: %s", what);
  return ECSIMD_HIP_ERR_BAD_ARG;
}
bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
bool overlaps(const void* a, const void* b) { return a == b; }
// An output that is one of the inputs (a null input is an argument the caller left out) or another output.
bool any_alias(std::initializer_list<const void*> out, std::initializer_list<const void*> in) {
  for (auto a = out.begin(); a != out.end(); ++a) {
    for (const void* b : in) if (b && overlaps(*a, b)) return true;
    for (auto b = a + 1; b != out.end(); ++b) if (overlaps(*a, *b)) return true;
  }
  return false;
}

// The way into every batched call, behind its argument checks: an empty batch is done, one launch covers at most 2^31 - 1 workgroups, the context's device is
// current.  ENTER_ANY_SIZE: the calls that go through the batch in chunks (or in a strided loop) and so take any n.
constexpr size_t MAX_LAUNCH = (size_t)0x7fffffff * BLOCK;
#define ENTER_IF(one_launch) do { \
    if (n == 0) return ECSIMD_HIP_OK; \
    if ((one_launch) && n > MAX_LAUNCH) return bad(ctx, "batch too large"); \
    hipError_t e0_ = hipSetDevice(ctx->device); if (e0_ != hipSuccess) return fail(ctx, e0_, "hipSetDevice"); } while (0)
#define ENTER() ENTER_IF(true)
#define ENTER_ANY_SIZE() ENTER_IF(false)
// for (first, m) over a batch of n in chunks of `chunk`: m is the chunk's length, the last one's may be shorter
#define FOR_CHUNKS(first, m, n, chunk) \
  for (size_t first = 0, m = (n) < (chunk) ? (n) : (chunk); first < (n); first += (chunk), m = (n) - first < (chunk) ? (n) - first : (chunk))
size_t chunk_of(size_t n, size_t most) { return n < most ? n : most; }

#define REQUIRE_CTX() do { if (!ctx) return ECSIMD_HIP_ERR_BAD_ARG; } while (0)
#define REQUIRE_PTR(p) do { if (!(p) && n) return bad(ctx, #p " is null"); if (!aligned16(p)) return bad(ctx, #p " is not 16-byte aligned"); } while (0)
// the y output of an affine result is optional (x-coordinate only); a Jacobian result needs it
#define REQUIRE_OUT_Y(p) do { if (!(flags & ECSIMD_HIP_OUT_AFFINE)) REQUIRE_PTR(p); else if ((p) && !aligned16(p)) return bad(ctx, #p " is not 16-byte aligned"); } while (0)
#define REQUIRE_CURVE() do { if (curve != ECSIMD_HIP_P256 && curve != ECSIMD_HIP_SECP256K1) return bad(ctx, "unknown curve"); } while (0)

// A curve registered at run time (id >= ECSIMD_HIP_FIRST_REGISTERED_CURVE): the generic kernels of k_gcurve.hip / k_gladder.hip take its record GC.
#define GENERIC_CURVE(call) do { if (curve >= ECSIMD_HIP_FIRST_REGISTERED_CURVE) { gcurve GC; if (!lookup_curve(curve, &GC)) return bad(ctx, "unknown curve id"); RUN(call); } } while (0)
// Enqueue one launcher call on the context's stream; report launch errors.
#define RUN(call) do { \
    ENTER(); \
    hipStream_t s = ctx->stream; (void)s; \
    call; \
    hipError_t e_ = hipGetLastError(); if (e_ != hipSuccess) return fail(ctx, e_, #call); \
    return ECSIMD_HIP_OK; } while (0)

void words_to_limbs(const uint32_t (&w)[8], uint64_t out[4]) {
  for (int i = 0; i < 4; ++i) out[i] = (uint64_t)w[2 * i] | ((uint64_t)w[2 * i + 1] << 32);
}
void limbs_to_words(const uint64_t l[4], uint32_t (&w)[8]) {
  for (int i = 0; i < 4; ++i) { w[2 * i] = (uint32_t)l[i]; w[2 * i + 1] = (uint32_t)(l[i] >> 32); }
}
launch::words8 words8_of(const uint64_t l[4]) { launch::words8 w; limbs_to_words(l, w.w); return w; }     // a 256-bit value as the kernels take it by value

// 256-bit host arithmetic (table plans, run-time moduli and curves): four 64-bit limbs, least significant first
struct u256 { uint64_t l[4]; };
bool u_geq(const u256& a, const u256& b) { for (int i = 3; i >= 0; --i) if (a.l[i] != b.l[i]) return a.l[i] > b.l[i]; return true; }
uint64_t u_sub(u256& r, const u256& a, const u256& b) {
  uint64_t bw = 0;
  for (int i = 0; i < 4; ++i) { const unsigned __int128 d = (unsigned __int128)a.l[i] - b.l[i] - bw; r.l[i] = (uint64_t)d; bw = (uint64_t)(d >> 64) & 1u; }
  return bw;
}
bool u_is_zero(const u256& a) { return !(a.l[0] | a.l[1] | a.l[2] | a.l[3]); }
bool u_eq(const u256& a, const u256& b) { return !memcmp(a.l, b.l, 32); }
u256 u_from(const uint64_t v[4]) { u256 r; memcpy(r.l, v, 32); return r; }

// Grow-only device scratch, ordered by the context's stream (synchronise before switching streams with
// ecsimd_hip_set_stream while a scratch-using call is in flight).  hipMalloc synchronises: callers that
// capture graphs warm the path up once.
bool capturing(ecsimd_hip_ctx* ctx) {
  hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(ctx->stream, &st) != hipSuccess) { (void)hipGetLastError(); return false; }
  return st != hipStreamCaptureStatusNone;
}
// The entry points that need the host -- they hand a value back, copy from or to memory that may be pageable, wait for the stream, allocate or time with
// events -- cannot be part of a capture, and a synchronisation on a capturing stream invalidates the whole capture.  They refuse BEFORE they touch the stream
// (include/ecsimd_hip.h, above ecsimd_hip_set_stream, lists them): nothing is enqueued and the caller's capture stays valid.
#define REFUSE_IN_CAPTURE(why) do { if (capturing(ctx)) return bad(ctx, why ": not inside a stream capture"); } while (0)
template <class T>
int ensure_block(ecsimd_hip_ctx* ctx, T*& block, size_t& have, size_t bytes, const char* during_capture, const char* what) {
  if (have >= bytes) return ECSIMD_HIP_OK;
  // Growing frees the old block: pointers a hipGraph captured earlier would dangle, and a capture in progress can neither
  // synchronise nor allocate.  The caller warms the path up at its largest batch BEFORE capturing (include/ecsimd_hip.h).
  if (capturing(ctx)) return bad(ctx, during_capture);
  hipError_t e = hipStreamSynchronize(ctx->stream);
  if (e == hipSuccess && block) e = hipFree(block);
  block = nullptr; have = 0;
  if (e == hipSuccess) e = hipMalloc(&block, bytes);
  if (e != hipSuccess) return fail(ctx, e, what);
  have = bytes;
  return ECSIMD_HIP_OK;
}
int ensure_workspace(ecsimd_hip_ctx* ctx, size_t bytes) {
  return ensure_block(ctx, ctx->workspace, ctx->workspace_bytes, bytes, "the context workspace would have to grow during stream capture: run this call once at the largest batch size before capturing", "workspace hipMalloc");
}
int ensure_valid(ecsimd_hip_ctx* ctx, size_t bytes) {
  return ensure_block(ctx, ctx->valid, ctx->valid_bytes, bytes, "the validity buffer would have to grow during stream capture: run this call once at the largest batch size before capturing", "validity buffer hipMalloc");
}

// A bump pointer over the workspace: limbs for m elements (32 B each), flag bytes for m elements (rounded up to 16), raw bytes.  A call carves twice with the
// same function: from a null base, where only `bytes` counts -- the size to ask ensure_workspace for --, and from ctx->workspace, which places the arrays.
struct carve { uint8_t* base; size_t bytes; };
carve carve_from(void* base) { return {static_cast<uint8_t*>(base), 0}; }
void* carve_bytes(carve& c, size_t bytes) { void* p = c.base ? c.base + c.bytes : nullptr; c.bytes += bytes; return p; }
uint64_t* carve_limbs(carve& c, size_t m) { return static_cast<uint64_t*>(carve_bytes(c, m * 32)); }
size_t flag_bytes(size_t m) { return (m + 15) / 16 * 16; }
uint8_t* carve_flags(carve& c, size_t m) { return static_cast<uint8_t*>(carve_bytes(c, flag_bytes(m))); }
struct jacobian { uint64_t *x, *y, *z; };
jacobian carve_jacobian(carve& c, size_t m) { jacobian j; j.x = carve_limbs(c, m); j.y = carve_limbs(c, m); j.z = carve_limbs(c, m); return j; }
// The Jacobian product of n lanes at the start of the workspace, grown to hold it: all that a product whose affine result goes to the caller's arrays needs.
size_t jacobian_bytes(size_t n) { carve c = carve_from(nullptr); (void)carve_jacobian(c, n); return c.bytes; }
int ensure_jacobian(ecsimd_hip_ctx* ctx, size_t n, jacobian* j) {
  int rc = ensure_workspace(ctx, jacobian_bytes(n));
  if (rc != ECSIMD_HIP_OK) return rc;
  carve c = carve_from(ctx->workspace); *j = carve_jacobian(c, n);
  return ECSIMD_HIP_OK;
}

// Window tables, produced with the (parity-checked) ladder kernel itself: odd multiples (2d + 1) 2^(bits w) G, 4 bits (64 x 8 entries), the
// constant-time comb's 5 bits (52 x 16), the signed comb's 7 bits (37 x 64) and the device-memory comb's BIG_WINDOW_BITS.
// ALG_CONSTANT_TIME reads EVERY entry of a window, so the best window is narrower than without it (profiles/r03/ab_constant_time_window_width.txt):
// 5 bits on both curves -- 52 windows x 16 entries, 51 additions, a 53 KB table, THREE 256-thread workgroups per CU (3 waves per SIMD, 146 VGPRs at most,
// no spill): P-256 326.0 M/s, secp256k1 323.0.  Measured against it: 4 bits (k_base_windowed<true>: 64 x 8, 63 additions) 280.7 / 278.1; 6 bits (43 x 32,
// one 1024-thread workgroup per CU) 324.2 / 279.5 (19 spills on secp256k1; at 768 threads 310.8 / 268.4); 7 bits (36 additions, 64 entries to read) 294.1 / 235.2.
// The other widths were removed.
constexpr int CT_WBITS = 5;
constexpr int SIGNED_WBITS = 7;     // 37 additions, 151 552 B of LDS (6 -> 43 additions, 88 064 B): measured faster
// The reference ladder's degenerate scalars (curve_group.h:189-218 as written: k forced odd, R0 + R1 = 2^i P): 0 and n end at Z = 0, n - 1,
// 2^256 - n - 1 and 2^256 - n meet n P = infinity inside a formula and return a wrong point.  k < 2^256; n = the group order.
// s = the three that return a point: {n - 1, 2^256 - n - 1, 2^256 - n}.
void ladder_degenerate_points(const u256& n, u256 (&s)[3]) {
  const u256 one = {{1, 0, 0, 0}}, zero = {{0, 0, 0, 0}};
  (void)u_sub(s[0], n, one); (void)u_sub(s[2], zero, n); (void)u_sub(s[1], s[2], one);
}
bool ladder_degenerate(const u256& n, const u256& k) {
  u256 s[3]; ladder_degenerate_points(n, s);
  return u_is_zero(k) || u_eq(k, n) || u_eq(k, s[0]) || u_eq(k, s[1]) || u_eq(k, s[2]);
}
// What an odd-digit comb with `bits`-bit windows asks of the ladder, for a built-in or a registered curve of order n >= 2^255 (ensure_window_table,
// ensure_gc_comb): ceil(256 / bits) windows x 2^(bits - 1) multipliers (2d + 1) 2^(bits w), then one more scalar, k*, whose point the kernel
// substitutes for its own sum (k_affine.inc comb_special: the one odd scalar at which the comb's last mixed addition meets R = T), and the 64-byte
// record {k*, 0} that goes behind the table.  Summed from the top (4 bits): k* = n - 2 (n mod 2^bits), and only if bit `bits` of k* is 0 (then its
// lowest digit is -(n mod 2^bits)); summed from the bottom (the others): k* = n - 2 (n mod 2^(bits (windows - 1))).
struct comb_plan {
  size_t table_entries, entries;        // entries = table_entries + 1: the point of k*
  std::vector<uint64_t> k;              // entries x 4 limbs: the ladder's scalars
  uint64_t kstar[8];                    // {k* (0: this kernel has no such scalar), 0}: read by comb_special
  bool negate_special;                  // the k* entry was computed as (n - k*) G: y -> p - y
};
int plan_comb(ecsimd_hip_ctx* ctx, const u256& n, int bits, comb_plan& P) {
  const int windows = (256 + bits - 1) / bits, per = 1 << (bits - 1);
  P.table_entries = (size_t)windows * per; P.entries = P.table_entries + 1;
  try { P.k.assign(P.entries * 4, 0); }                        // up to 218 MB of host memory (20-bit windows): nothing may throw across the C ABI
  catch (...) { return bad(ctx, "window table: out of host memory"); }
  u256 dg[3]; ladder_degenerate_points(n, dg);
  for (int w = 0; w < windows; ++w)
    for (int d = 0; d < per; ++d) {
      uint64_t* e = &P.k[((size_t)w * per + d) * 4];
      const int pos = bits * w, limb = pos / 64, off = pos % 64;
      const unsigned __int128 v = (unsigned __int128)(2u * (unsigned)d + 1u) << off;
      if (limb + 1 >= 4 && (uint64_t)(v >> 64) != 0) { e[0] = 1; continue; }        // (2d + 1) 2^pos >= 2^256: beyond the top digit's range, never read
      e[limb] = (uint64_t)v;
      if (limb + 1 < 4) e[limb + 1] = (uint64_t)(v >> 64);
      const u256 m = u_from(e);                                                    // (odd times a power of two: never 0 or n)
      if (u_eq(m, dg[0]) || u_eq(m, dg[1]) || u_eq(m, dg[2])) return bad(ctx, "window table: a table multiplier is one of the ladder's degenerate scalars on this curve");
    }
  const int low = bits == 4 ? bits : bits * (windows - 1);
  u256 m = n, m2, ks;
  for (int l = 0; l < 4; ++l) { const int lo = 64 * l; if (low <= lo) m.l[l] = 0; else if (low < lo + 64) m.l[l] &= (1ull << (low - lo)) - 1ull; }
  for (int l = 3; l > 0; --l) m2.l[l] = (m.l[l] << 1) | (m.l[l - 1] >> 63);
  m2.l[0] = m.l[0] << 1;                                                           // 2 m (m < 2^255)
  const bool have = !u_sub(ks, n, m2) && !u_is_zero(ks) && (bits != 4 || ((ks.l[0] >> bits) & 1u) == 0);
  for (int l = 0; l < 8; ++l) P.kstar[l] = (have && l < 4) ? ks.l[l] : 0;
  u256 mult = have ? ks : u256{{1, 0, 0, 0}};                                      // without a k*: any scalar, the point is never used
  P.negate_special = false;
  // k* G comes from the reference ladder, and the ladder has degenerate scalars of its own.  The 5-bit comb summed from the
  // bottom has k* = n - 2 (n mod 2^255) = 2^256 - n -- one of them: there the ladder multiplies by n - k* instead (never degenerate when
  // k* is: checked) and the entry's y is negated after the conversion.
  if (have && ladder_degenerate(n, ks)) {
    (void)u_sub(mult, n, ks);
    if (ladder_degenerate(n, mult)) return bad(ctx, "window table: neither k* nor n - k* is a scalar the ladder multiplies correctly");
    P.negate_special = true;
  }
  for (int l = 0; l < 4; ++l) P.k[P.table_entries * 4 + l] = mult.l[l];
  return ECSIMD_HIP_OK;
}
u256 order_of(int curve) {
  uint64_t l[4];
  words_to_limbs(curve == ECSIMD_HIP_P256 ? curve_order<CURVE_P256>::N : curve_order<CURVE_SECP256K1>::N, l);
  return u_from(l);
}
static_assert(launch::FIXED4_ENTRIES == 8, "plan_comb: the 4-bit comb's table is 64 x 8");
int ensure_window_table(ecsimd_hip_ctx* ctx, int curve, int bits) {
  uint32_t** slot = (bits == 4) ? &ctx->window_table[curve] : (bits == launch::BIG_WINDOW_BITS) ? &ctx->window16_table[curve] : (bits == CT_WBITS) ? &ctx->windowct_table[curve] : &ctx->window6_table[curve];
  if (*slot) return ECSIMD_HIP_OK;
  comb_plan P;
  int rc = plan_comb(ctx, order_of(curve), bits, P);
  if (rc != ECSIMD_HIP_OK) return rc;
  const size_t entries = P.entries;
  // The build needs 6 x entries x 32 B of scratch (1.3 GB for the 20-bit table): a TEMPORARY block freed below, not the
  // context's grow-only workspace -- a caller that verifies one signature must not keep 1.3 GB pinned for it.
  if (capturing(ctx)) return bad(ctx, "a window table would have to be built during stream capture: run this call once before capturing");
  uint64_t* kd = nullptr;
  uint32_t* table = nullptr;
  hipError_t e = hipMalloc(&kd, 6 * entries * 32);
  if (e == hipSuccess) e = hipMalloc(&table, (entries + 1) * 64);      // + the record that holds k*
  uint64_t* tx = kd + entries * 4; uint64_t* ty = tx + entries * 4;
  if (e == hipSuccess) e = hipMemcpyAsync(kd, P.k.data(), entries * 32, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);          // P.k must outlive the copy
  if (e == hipSuccess) {   // ladder (Jacobian, fast domain) into scratch, then affine classical (x, y)
    uint64_t* jx = ty + entries * 4; uint64_t* jy = jx + entries * 4; uint64_t* jz = jy + entries * 4;
    launch::scalar_mult(ctx->stream, curve, kd, 4, nullptr, nullptr, jx, jy, jz, entries, ECSIMD_HIP_OUT_AFFINE);
    launch::to_affine_batched(ctx->stream, curve, jx, jy, jz, tx, ty, entries, true);
    if (P.negate_special) launch::field_unop(ctx->stream, curve, launch::F_OPPOSITE, ty + P.table_entries * 4, ty + P.table_entries * 4, 1);   // -(x, y) = (x, p - y)
    if (bits == launch::BIG_WINDOW_BITS) launch::pack_table_big(ctx->stream, curve, tx, ty, table);
    else if (bits == 4) launch::pack_table(ctx->stream, curve, tx, ty, table);
    else launch::pack_table_signed(ctx->stream, curve, bits, tx, ty, table);
    e = hipMemcpyAsync(table + entries * 16, P.kstar, 64, hipMemcpyHostToDevice, ctx->stream);
  }
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e == hipSuccess) e = hipGetLastError();
  (void)hipFree(kd);
  if (e != hipSuccess) { (void)hipFree(table); return fail(ctx, e, "window table build"); }
  *slot = table;
  return ECSIMD_HIP_OK;
}

// The kernel instance an entry point runs: the API curve, or its reference-square twin (field.cuh) when the
// context option or the call's ECSIMD_HIP_REF_SQUARE_COMPAT flag asks for the reference's bits.
bool wants_compat(const ecsimd_hip_ctx* ctx, int flags = 0) { return ctx->ref_square || (flags & ECSIMD_HIP_REF_SQUARE_COMPAT); }
int instance(const ecsimd_hip_ctx* ctx, int curve, int flags = 0) {
  return wants_compat(ctx, flags) ? curve + (CURVE_P256_REFSQR - CURVE_P256) : curve;
}
static_assert(CURVE_SECP256K1_REFSQR - CURVE_SECP256K1 == CURVE_P256_REFSQR - CURVE_P256, "instance() adds one offset");
// What every call that is not the reference's own ladder or formulas answers to wants_compat(); what = the call (nullptr: the message names none).
int refuse_compat(ecsimd_hip_ctx* ctx, const char* what) {
  snprintf(ctx->err, sizeof ctx->err, "bad argument: %s%snot the reference's algorithm: no ECSIMD_HIP_REF_SQUARE_COMPAT form", what ? what : "", what ? " is " : "");
  return ECSIMD_HIP_ERR_BAD_ARG;
}
#define NO_COMPAT(what) do { if (wants_compat(ctx, flags)) return refuse_compat(ctx, what); } while (0)

// ---- the steps the entry points share
// The group order of a built-in curve, as the scalar-field kernels (gmod) and the others (words) take it.
struct group_order { gmod N; launch::words8 words; };
bool lookup_modulus(int id, gmod* out);          // the modulus registry, below
int builtin_order(ecsimd_hip_ctx* ctx, int curve, group_order* out) {
  if (!lookup_modulus(curve == ECSIMD_HIP_P256 ? ECSIMD_HIP_FIELD_P256_ORDER : ECSIMD_HIP_FIELD_SECP256K1_ORDER, &out->N)) return bad(ctx, "group order missing from the registry");
  for (int i = 0; i < 8; ++i) out->words.w[i] = out->N.p[i];
  return ECSIMD_HIP_OK;
}

// k G for SECRET k on a built-in curve: the constant-time 5-bit comb (ensure_window_table(CT_WBITS) first), then the simultaneous inversion; y == nullptr: x only.
// Stream-ordered, nothing read back.  The Jacobian product j and, where x / y lie in the workspace, the affine point are the caller's to wipe: with a public
// function of the point (ECDSA's r), the Z of the unnormalised k G gives bits of k away (the projective-coordinate leak), and the block outlives the call
// (grow-only, hipFree does not wipe).
void secret_base_product(ecsimd_hip_ctx* ctx, int curve, const uint64_t* k, const jacobian& j, uint64_t* x, uint64_t* y, size_t m) {
  launch::base_windowed_signed(ctx->stream, curve, k, ctx->windowct_table[curve], j.x, j.y, j.z, m, true);      // k >= n is reduced by the comb; the caller's kernel refuses the lane
  launch::to_affine_batched(ctx->stream, curve, j.x, j.y, j.z, x, y, m, true);
}
// The end of a scope that left secrets in the first `bytes` of the workspace (its carve's total): zero them on the same stream, behind the scope's launches and
// whatever those said -- `launches` is their hipGetLastError().  Returns the first error of the two.
hipError_t wipe_workspace(ecsimd_hip_ctx* ctx, size_t bytes, hipError_t launches) {
  const hipError_t wiped = hipMemsetAsync(ctx->workspace, 0, bytes, ctx->stream);
  return launches != hipSuccess ? launches : wiped;
}

// u G for PUBLIC u on a built-in curve: the 20-bit comb in device memory (436 MB per curve, built on first use) once that table exists or a batch of `batch`
// elements is large enough to pay for building it; smaller batches take the signed 7-bit comb in LDS.  Ensures the table, then launches m lanes of it; u == nullptr:
// the table only, for a caller that sizes its workspace and launches its front end before its chunk loop gets here.
constexpr size_t BIG_TABLE_WORTH_IT = (size_t)1 << 16;
int public_base_product(ecsimd_hip_ctx* ctx, int curve, size_t batch, const uint64_t* u = nullptr, const jacobian* j = nullptr, size_t m = 0) {
  const bool big = ctx->window16_table[curve] != nullptr || batch >= BIG_TABLE_WORTH_IT;
  int rc = ensure_window_table(ctx, curve, big ? launch::BIG_WINDOW_BITS : SIGNED_WBITS);
  if (rc != ECSIMD_HIP_OK || !u) return rc;
  if (big) launch::base_windowed_big(ctx->stream, curve, u, ctx->window16_table[curve], j->x, j->y, j->z, m);
  else launch::base_windowed_signed(ctx->stream, curve, u, ctx->window6_table[curve], j->x, j->y, j->z, m, false);
  return ECSIMD_HIP_OK;
}

// The reference ladder, then (for OUT_AFFINE) one simultaneous inversion over the whole batch.
int run_ladder(ecsimd_hip_ctx* ctx, int curve, const uint64_t* k, int k_stride, const uint64_t* x, const uint64_t* y,
               uint64_t* ox, uint64_t* oy, uint64_t* oz, size_t n, int flags) {
  ENTER();
  hipError_t e;
  if ((flags & ECSIMD_HIP_OUT_AFFINE) && oy == nullptr && curve == ECSIMD_HIP_P256 && instance(ctx, curve, flags) == curve) {
    // x only: the ladder without Z (point.cuh scalar_mult_ladder_x) -- 8M + 6S per bit instead of 9M + 7S
    int rc = ensure_workspace(ctx, launch::scalar_mult_x_scratch_bytes(n));
    if (rc != ECSIMD_HIP_OK) return rc;
    launch::point_launch<CURVE_P256>::scalar_mult_x(ctx->stream, k, k_stride, x, y, ox, ctx->workspace, n, flags);
    e = hipGetLastError();
    return e == hipSuccess ? ECSIMD_HIP_OK : fail(ctx, e, "scalar_mult (x only) launch");
  }
  if (flags & ECSIMD_HIP_OUT_AFFINE) {
    jacobian j; int rc = ensure_jacobian(ctx, n, &j);
    if (rc != ECSIMD_HIP_OK) return rc;
    const int cv = instance(ctx, curve, flags);
    launch::scalar_mult(ctx->stream, cv, k, k_stride, x, y, j.x, j.y, j.z, n, flags);
    // reference-square instances: to_affine() per element with the reference's own power ladder (gfp.h:42-44)
    if (cv != curve) launch::to_affine(ctx->stream, cv, j.x, j.y, j.z, ox, oy, n);
    else launch::to_affine_batched(ctx->stream, curve, j.x, j.y, j.z, ox, oy, n, true);
  } else {
    launch::scalar_mult(ctx->stream, instance(ctx, curve, flags), k, k_stride, x, y, ox, oy, oz, n, flags);
  }
  e = hipGetLastError();
  return e == hipSuccess ? ECSIMD_HIP_OK : fail(ctx, e, "scalar_mult launch");
}

bool lookup_curve(int id, gcurve* out);          // the curve registry, below
// The same for a curve registered at run time: flags BASE_* | OUT_* | LADDER_RADIX32 | REF_SQUARE_COMPAT; the table-driven ALG_* algorithms exist for the
// two built-in curves only.  x == nullptr: the curve's generator.
int run_gcomb(ecsimd_hip_ctx* ctx, int curve, const uint64_t* k, uint64_t* ox, uint64_t* oy, size_t n, int flags);
constexpr int GC_NOT_TAKEN = -1000;
int gc_small_base(ecsimd_hip_ctx* ctx, int curve, const uint64_t* k, uint64_t* ox, uint64_t* oy, size_t n, int flags);
int run_gvarwin(ecsimd_hip_ctx* ctx, int curve, const uint64_t* k, int k_stride, const uint64_t* x, const uint64_t* y, uint64_t* ox, uint64_t* oy, size_t n, int flags, size_t reserve);
int run_gladder(ecsimd_hip_ctx* ctx, int curve, const uint64_t* k, int k_stride, const uint64_t* x, const uint64_t* y,
                uint64_t* ox, uint64_t* oy, uint64_t* oz, size_t n, int flags) {
  gcurve GC; if (!lookup_curve(curve, &GC)) return bad(ctx, "unknown curve id");
  if (x == nullptr && k_stride == 4 && (flags & ECSIMD_HIP_ALG_WINDOWED) && !(flags & (ECSIMD_HIP_ALG_WINDOWED_SIGNED | ECSIMD_HIP_ALG_WINDOWED_BIG | ECSIMD_HIP_ALG_NO_ENDOMORPHISM)))
    return run_gcomb(ctx, curve, k, ox, oy, n, flags);          // k G from the generator's table in LDS (k_gcomb.hip)
  if (x == nullptr && k_stride == 4 && (flags & ECSIMD_HIP_ALG_WINDOWED_SIGNED) && !(flags & (ECSIMD_HIP_ALG_WINDOWED | ECSIMD_HIP_ALG_WINDOWED_BIG | ECSIMD_HIP_ALG_NO_ENDOMORPHISM | ECSIMD_HIP_ALG_CONSTANT_TIME)))
    return run_gcomb(ctx, curve, k, ox, oy, n, flags);          // ... from the signed 7-bit comb (public scalars)
  if (x == nullptr && k_stride == 4 && (flags & ECSIMD_HIP_ALG_WINDOWED_BIG) && !(flags & (ECSIMD_HIP_ALG_WINDOWED | ECSIMD_HIP_ALG_WINDOWED_SIGNED | ECSIMD_HIP_ALG_NO_ENDOMORPHISM | ECSIMD_HIP_ALG_CONSTANT_TIME)))
    return run_gcomb(ctx, curve, k, ox, oy, n, flags);          // ... from the 20-bit comb in device memory (public scalars)
  if (x != nullptr && (flags & ECSIMD_HIP_ALG_WINDOWED) && !(flags & (ECSIMD_HIP_ALG_WINDOWED_SIGNED | ECSIMD_HIP_ALG_WINDOWED_BIG | ECSIMD_HIP_ALG_NO_ENDOMORPHISM)))
    return run_gvarwin(ctx, curve, k, k_stride, x, y, ox, oy, n, flags, 0);   // k P from the lane's own table of odd multiples (k_gvarwin.hip); ALG_CONSTANT_TIME: every entry read in every window
  if (flags & (ECSIMD_HIP_ALG_WINDOWED | ECSIMD_HIP_ALG_WINDOWED_SIGNED | ECSIMD_HIP_ALG_WINDOWED_BIG | ECSIMD_HIP_ALG_NO_ENDOMORPHISM | ECSIMD_HIP_ALG_CONSTANT_TIME))
    return bad(ctx, "a registered curve has the reference's ladder, ALG_WINDOWED [| ALG_CONSTANT_TIME] for its generator and for a variable base, and ALG_WINDOWED_SIGNED / ALG_WINDOWED_BIG for its generator: the other combinations (the GLV split, constant-time forms of the signed and big combs) exist for P-256 and secp256k1 or not at all");
  ENTER();
  const bool ref = wants_compat(ctx, flags);
  const int lf = (flags & (ECSIMD_HIP_BASE_MGRY | ECSIMD_HIP_LADDER_RADIX32)) | (ref ? ECSIMD_HIP_REF_SQUARE_COMPAT : 0);
  if (flags & ECSIMD_HIP_OUT_AFFINE) {
    jacobian j; int rc = ensure_jacobian(ctx, n, &j);
    if (rc != ECSIMD_HIP_OK) return rc;
    launch::gc_scalar_mult(ctx->stream, GC, k, k_stride, x, y, j.x, j.y, j.z, n, lf);
    if (ref) launch::gc_to_affine(ctx->stream, GC, j.x, j.y, j.z, ox, oy, n, true);       // the reference's own power ladder per element (gfp.h:42-44)
    else launch::gc_to_affine_batched(ctx->stream, GC, j.x, j.y, j.z, ox, oy, n);
  } else {
    launch::gc_scalar_mult(ctx->stream, GC, k, k_stride, x, y, ox, oy, oz, n, lf);
  }
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? ECSIMD_HIP_OK : fail(ctx, e, "scalar_mult (registered curve) launch");
}

// Variable-base windowed multiplication in chunks of VARWIN_CHUNK lanes (1 408 B of scratch per lane: the
// per-lane tables live in HBM).  `reserve` bytes at the start of the workspace stay untouched (double_scalar_mult).
constexpr size_t VARWIN_CHUNK = (size_t)1 << 22;
int run_varwin(ecsimd_hip_ctx* ctx, int curve, const uint64_t* k, int k_stride, const uint64_t* x, const uint64_t* y,
               uint64_t* ox, uint64_t* oy, size_t n, int flags, size_t reserve) {
  ENTER_ANY_SIZE();
  const size_t chunk = chunk_of(n, VARWIN_CHUNK);
  int rc = ensure_workspace(ctx, reserve + launch::varwin_scratch_bytes(chunk));
  if (rc != ECSIMD_HIP_OK) return rc;
  uint64_t* scratch = ctx->workspace + reserve / 8;
  FOR_CHUNKS(first, m, n, chunk)
    launch::varwin_scalar_mult(ctx->stream, curve, k + (size_t)k_stride * first, k_stride, x + 4 * first, y + 4 * first, flags, scratch, ox + 4 * first, oy ? oy + 4 * first : nullptr, m);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? ECSIMD_HIP_OK : fail(ctx, e, "scalar_mult (windowed) launch");
}
}  // namespace

// ---- the small-batch route of scalar_mult_base (see ecsimd_hip_scalar_mult_base)
namespace {
constexpr size_t SMALL_BASE_MAX = (size_t)1 << 16;
// A stream under capture can neither build the comb's table nor the record below: such a call keeps the ladder (and stays capturable).
bool capturing_needs_build(ecsimd_hip_ctx* ctx, int curve) {
  return capturing(ctx) && (!ctx->windowct_table[curve] || !ctx->base_special[curve]);
}
int ensure_base_special(ecsimd_hip_ctx* ctx, int curve) {
  if (ctx->base_special[curve]) return ECSIMD_HIP_OK;
  u256 s3[3]; ladder_degenerate_points(order_of(curve), s3);
  uint64_t host[12];
  for (int j = 0; j < 3; ++j) for (int l = 0; l < 4; ++l) host[4 * j + l] = s3[j].l[l];
  uint64_t* rec = nullptr; uint64_t* tmp = nullptr;
  hipError_t e = hipMalloc(&rec, 9 * 32);
  if (e == hipSuccess) e = hipMalloc(&tmp, 9 * 32);               // Jacobian scratch of the three ladders
  if (e == hipSuccess) e = hipMemcpyAsync(rec, host, 3 * 32, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);     // `host` is on this stack frame
  if (e == hipSuccess) {
    launch::scalar_mult(ctx->stream, curve, rec, 4, nullptr, nullptr, tmp, tmp + 12, tmp + 24, 3, ECSIMD_HIP_OUT_AFFINE);    // the ladder, fast domain
    launch::to_affine_batched(ctx->stream, curve, tmp, tmp + 12, tmp + 24, rec + 12, rec + 24, 3, true);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  }
  (void)hipFree(tmp);
  if (e != hipSuccess) { (void)hipFree(rec); return fail(ctx, e, "base_special build"); }
  ctx->base_special[curve] = rec;
  return ECSIMD_HIP_OK;
}
}  // namespace

// ================================================================== run-time moduli
// The reference's field layer is generic in the modulus type P (mgry_mul.h:84-121, mgry_csts.h:15-35, gfp.h:17-115): a caller
// instantiates it for any odd 256-bit P at compile time.  Here the same genericity is a run-time registry: a field id names a
// modulus, the host derives what mgry_constants<WBN, P> / mgry_mul_constants derive (R, R^2, -R mod p, m') plus the division-step
// constants, and the generic kernels of k_gfield.hip take the record as a kernel argument.  Ids 0, 1 are the curve primes (their
// special-form kernels, field.cuh); 2, 3 the two group orders; 4... whatever ecsimd_hip_register_modulus was given.  Process-wide,
// append-only, guarded by one mutex (registration is rare; lookups copy 236 bytes).
namespace {
void u_dbl_mod(u256& a, const u256& p) {                       // a < p  ->  2a mod p
  const uint64_t top = a.l[3] >> 63;
  for (int i = 3; i > 0; --i) a.l[i] = (a.l[i] << 1) | (a.l[i - 1] >> 63);
  a.l[0] <<= 1;
  if (top || u_geq(a, p)) { u256 t; (void)u_sub(t, a, p); a = t; }
}
void u_words(uint32_t (&w)[8], const u256& v) { limbs_to_words(v.l, w); }
gmod make_gmod(const uint64_t pl[4], uint32_t flags) {
  gmod M; memset(&M, 0, sizeof M);
  u256 p; for (int i = 0; i < 4; ++i) p.l[i] = pl[i];
  u_words(M.p, p);
  u256 t = {{1, 0, 0, 0}};                                    // 1 < p (p >= 3)
  for (int i = 0; i < 256; ++i) u_dbl_mod(t, p);
  u_words(M.r, t);                                            // R mod p            mgry_csts.h:20 (cbn::div there)
  { u256 nr; (void)u_sub(nr, p, t); u_words(M.negr, nr); }    // -R mod p = p - (R mod p), R mod p in [1, p)   mgry_csts.h:24
  for (int i = 0; i < 256; ++i) u_dbl_mod(t, p);
  u_words(M.rsq, t);                                          // R^2 mod p          mgry_csts.h:21
  for (int i = 0; i < 256; ++i) u_dbl_mod(t, p);
  u_words(M.r3, t);                                           // R^3 mod p
  { u256 two = {{2, 0, 0, 0}}, e; (void)u_sub(e, p, two); u_words(M.pm2, e); }                                     // gfp.h:79-81
  { unsigned __int128 c = 1; u256 q; for (int i = 0; i < 4; ++i) { c += p.l[i]; q.l[i] = (uint64_t)c; c >>= 64; }   // (p + 1) / 4, the carry of p + 1 kept
    u256 h; for (int i = 0; i < 4; ++i) h.l[i] = (q.l[i] >> 2) | ((i < 3 ? q.l[i + 1] : (uint64_t)c) << 62); u_words(M.psqrt, h); }
  for (int i = 0; i < 9; ++i) {                               // p in 30-bit limbs (the top one holds bits 240..255)
    const int bit = 30 * i, limb = bit / 64, off = bit % 64;
    uint64_t v = p.l[limb] >> off;
    if (off > 34 && limb + 1 < 4) v |= p.l[limb + 1] << (64 - off);
    M.p30[i] = (int32_t)(v & (i < 8 ? 0x3fffffffu : 0xffffu));
  }
  uint32_t p0 = (uint32_t)p.l[0], inv = p0;                   // p^-1 mod 2^32 by Newton iteration (mgry_mul.h:33-38 uses cbn::mod_inv)
  for (int i = 0; i < 5; ++i) inv *= 2u - p0 * inv;
  M.pinv30 = inv & 0x3fffffffu;
  M.mprime = 0u - inv;
  M.flags = (flags & GMOD_PRIME) | ((p0 & 3u) == 3u ? GMOD_3MOD4 : 0u);
  return M;
}
struct modulus_registry {
  std::mutex mu;
  std::vector<gmod> mods;                                     // index = field id - 2
  modulus_registry() {
    uint64_t n[4];
    words_to_limbs(curve_order<CURVE_P256>::N, n); mods.push_back(make_gmod(n, GMOD_PRIME));
    words_to_limbs(curve_order<CURVE_SECP256K1>::N, n); mods.push_back(make_gmod(n, GMOD_PRIME));
  }
};
modulus_registry& registry() { static modulus_registry r; return r; }
constexpr int FIRST_FIELD_ID = 2, MAX_FIELDS = 4096;
// the record of field id `id` (>= 2); false if there is none
bool lookup_curve(int id, gcurve* out);
bool lookup_modulus(int id, gmod* out) {
  if (id >= ECSIMD_HIP_FIRST_REGISTERED_CURVE) { gcurve G; if (!lookup_curve(id, &G)) return false; *out = G.F; return true; }     // a registered curve's id names its prime's field
  modulus_registry& r = registry();
  std::lock_guard<std::mutex> g(r.mu);
  if (id < FIRST_FIELD_ID || (size_t)(id - FIRST_FIELD_ID) >= r.mods.size()) return false;
  *out = r.mods[id - FIRST_FIELD_ID];
  return true;
}
// ================================================================== run-time curves (round 5)
// The reference's group layer is a template over ANY curve type -- curve_group<Curve> for every Curve with bn_type, P, A, B, Gx, Gy (curve.h:12-15,
// curve_group.h:20-33) over a field GFp<WBN, P> that needs p = 3 mod 4 (gfp.h:84).  Here a curve is a run-time record with an id >= FIRST_CURVE_ID:
// the host derives what the templates derive (the field's constants as for a modulus, Am = a R, Bm = b R: curve_group.h:31-32) plus the 29-bit-limb
// constants of the ladder's loop, and the generic kernels (k_gcurve.hip, k_gladder.hip) take the 512-byte record as a kernel argument.
constexpr int FIRST_CURVE_ID = ECSIMD_HIP_FIRST_REGISTERED_CURVE, MAX_CURVES = 4096;
u256 u_add_mod(const u256& a, const u256& b, const u256& p) {          // a, b < p
  u256 s; unsigned __int128 c = 0;
  for (int i = 0; i < 4; ++i) { c += (unsigned __int128)a.l[i] + b.l[i]; s.l[i] = (uint64_t)c; c >>= 64; }
  if ((uint64_t)c || u_geq(s, p)) { u256 t; (void)u_sub(t, s, p); s = t; }
  return s;
}
u256 u_mul_mod(const u256& a, const u256& b, const u256& p) {          // a, b < p: double-and-add (registration is rare)
  u256 r = {{0, 0, 0, 0}};
  for (int i = 255; i >= 0; --i) { u_dbl_mod(r, p); if ((b.l[i >> 6] >> (i & 63)) & 1u) r = u_add_mod(r, a, p); }
  return r;
}
u256 u_shl_mod(u256 a, int bits, const u256& p) { for (int i = 0; i < bits; ++i) u_dbl_mod(a, p); return a; }
void u_limbs29(int32_t (&out)[9], const u256& v) {                      // tight 29-bit limbs (tools/radix29_model.py to_limbs)
  for (int i = 0; i < 9; ++i) {
    const int bit = 29 * i, limb = bit / 64, off = bit % 64;
    uint64_t w = v.l[limb] >> off;
    if (off > 64 - 29 && limb + 1 < 4) w |= v.l[limb + 1] << (64 - off);
    out[i] = (int32_t)(w & (i < 8 ? 0x1fffffffu : 0xffffffu));
  }
}
struct curve_record { gcurve G; u256 a, b, n; bool has_order; gmod N; bool ecdsa_ok; bool prime_order; bool order_wrong; };   // order_wrong: n looks like THE group order (prime, in p's Hasse interval) and n G != O
// What a per-lane window table of a VARIABLE base needs beyond the recoding's n >= 2^255: every point on the curve but infinity has order exactly n, so that
// "no addition inside the loop is exceptional" -- a statement about scalars modulo the ORDER OF THE POINT -- holds for every valid input, not only for
// multiples of the generator.  That is: the group has order n (n divides #E and lies in p's Hasse interval, where no second multiple of an n >= 2^255 fits)
// and n is prime.  Checked once per registration on the host: the Hasse test exactly ((|n - p - 1| / 2 rounded up)^2 <= p; conservative by at most one
// at the interval's edge), primality by Miller-Rabin on 16 fixed bases -- a guard against a wrong parameter set, not against a forged one (the caller vouches
// for p's primality in the same way).
bool u_hasse(const u256& n, const u256& p) {
  u256 p1 = p; { int i = 0; while (i < 4 && ++p1.l[i] == 0) ++i; if (i == 4) return false; }
  u256 d; if (u_geq(n, p1)) (void)u_sub(d, n, p1); else (void)u_sub(d, p1, n);
  if (d.l[3] || d.l[2] > 1) return false;                              // 2 sqrt(p) < 2^129
  unsigned __int128 e = ((unsigned __int128)d.l[1] << 64) | d.l[0];
  e = ((e >> 1) | ((unsigned __int128)d.l[2] << 127)) + (d.l[0] & 1);   // ceil(d / 2) <= 2^128
  if (e == 0 && (d.l[2] | d.l[1] | d.l[0])) return false;              // (it was 2^128: beyond sqrt(p))
  const uint64_t e0 = (uint64_t)e, e1 = (uint64_t)(e >> 64);
  const unsigned __int128 lo = (unsigned __int128)e0 * e0, mid = (unsigned __int128)e0 * e1, hi = (unsigned __int128)e1 * e1;
  u256 sq; unsigned __int128 c;
  sq.l[0] = (uint64_t)lo;
  c = (lo >> 64) + (uint64_t)mid + (uint64_t)mid; sq.l[1] = (uint64_t)c;
  c = (c >> 64) + (mid >> 64) + (mid >> 64) + (uint64_t)hi; sq.l[2] = (uint64_t)c;
  c = (c >> 64) + (hi >> 64); sq.l[3] = (uint64_t)c;
  if (c >> 64) return false;
  return u_geq(p, sq);
}
bool u_probable_prime(const u256& n) {
  if (!(n.l[0] & 1u) || (!(n.l[3] | n.l[2] | n.l[1]) && n.l[0] < 128)) return false;       // (the callers' n is odd and >= 2^255)
  const u256 one = {{1, 0, 0, 0}};
  u256 nm1; (void)u_sub(nm1, n, one);
  int s = 0; u256 d = nm1;
  while (!(d.l[0] & 1u)) { for (int i = 0; i < 3; ++i) d.l[i] = (d.l[i] >> 1) | (d.l[i + 1] << 63); d.l[3] >>= 1; ++s; }
  static const uint64_t bases[16] = {2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37, 41, 43, 47, 53};
  for (uint64_t b : bases) {
    const u256 a = {{b, 0, 0, 0}};
    u256 x = one;
    for (int i = 255; i >= 0; --i) { x = u_mul_mod(x, x, n); if ((d.l[i >> 6] >> (i & 63)) & 1u) x = u_mul_mod(x, a, n); }
    if (u_eq(x, one) || u_eq(x, nm1)) continue;
    bool witness = true;
    for (int r = 1; r < s && witness; ++r) { x = u_mul_mod(x, x, n); if (u_eq(x, nm1)) witness = false; }
    if (witness) return false;
  }
  return true;
}
// n G = O on the host, once per registration: Jacobian double-and-add from the top bit over u_mul_mod (Z = 0: infinity; ~6 000 products, a few ms).
// A prime n in p's Hasse interval that does not annihilate G is a wrong parameter set, and the comb and the window loop recode modulo n.
u256 u_sub_mod(const u256& a, const u256& b, const u256& p) { u256 t; if (u_is_zero(b)) return a; (void)u_sub(t, p, b); return u_add_mod(a, t, p); }
bool u_order_annihilates(const u256& gx, const u256& gy, const u256& a, const u256& p, const u256& n) {
  const u256 zero = {{0, 0, 0, 0}}, one = {{1, 0, 0, 0}};
  u256 X = zero, Y = one, Z = zero;
  auto M = [&](const u256& u, const u256& v) { return u_mul_mod(u, v, p); };
  auto dbl = [&]() {
    if (u_is_zero(Z)) return;
    const u256 YY = M(Y, Y), ZZ = M(Z, Z), XX = M(X, X);
    u256 S = M(X, YY); u_dbl_mod(S, p); u_dbl_mod(S, p);                                       // 4 X Y^2
    const u256 Mm = u_add_mod(u_add_mod(u_add_mod(XX, XX, p), XX, p), M(a, M(ZZ, ZZ)), p);     // 3 X^2 + a Z^4
    const u256 X3 = u_sub_mod(M(Mm, Mm), u_add_mod(S, S, p), p);
    u256 Y4 = M(YY, YY); u_dbl_mod(Y4, p); u_dbl_mod(Y4, p); u_dbl_mod(Y4, p);                  // 8 Y^4
    u256 Z3 = M(Y, Z); u_dbl_mod(Z3, p);                                                       // (Y = 0: a point of order two, Z3 = 0)
    Y = u_sub_mod(M(Mm, u_sub_mod(S, X3, p)), Y4, p); X = X3; Z = Z3;
  };
  for (int i = 255; i >= 0; --i) {
    dbl();
    if (!((n.l[i >> 6] >> (i & 63)) & 1u)) continue;
    if (u_is_zero(Z)) { X = gx; Y = gy; Z = one; continue; }
    const u256 ZZ = M(Z, Z), H = u_sub_mod(M(gx, ZZ), X, p), R = u_sub_mod(M(gy, M(Z, ZZ)), Y, p);
    if (u_is_zero(H)) { if (u_is_zero(R)) dbl(); else Z = zero; continue; }                     // the same point: double; opposite points: infinity
    const u256 HH = M(H, H), HHH = M(H, HH), V = M(X, HH);
    const u256 X3 = u_sub_mod(u_sub_mod(M(R, R), HHH, p), u_add_mod(V, V, p), p);
    Y = u_sub_mod(M(R, u_sub_mod(V, X3, p)), M(Y, HHH), p); X = X3; Z = M(Z, H);
  }
  return u_is_zero(Z);
}
struct curve_registry { std::mutex mu; std::vector<curve_record> curves; };
curve_registry& curves() { static curve_registry r; return r; }
bool lookup_curve(int id, gcurve* out) {
  curve_registry& r = curves();
  std::lock_guard<std::mutex> g(r.mu);
  if (id < FIRST_CURVE_ID || (size_t)(id - FIRST_CURVE_ID) >= r.curves.size()) return false;
  *out = r.curves[id - FIRST_CURVE_ID].G;
  return true;
}
bool lookup_curve_record(int id, curve_record* out) {
  curve_registry& r = curves();
  std::lock_guard<std::mutex> g(r.mu);
  if (id < FIRST_CURVE_ID || (size_t)(id - FIRST_CURVE_ID) >= r.curves.size()) return false;
  *out = r.curves[id - FIRST_CURVE_ID];
  return true;
}
}  // namespace

extern "C" {

const char* ecsimd_hip_version(void) { return "ecsimd-hip 0.1 (gfx950)"; }

int ecsimd_hip_init(int device, ecsimd_hip_ctx** out) {
  if (!out) return ECSIMD_HIP_ERR_BAD_ARG;
  *out = nullptr;
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0 || device < 0 || device >= count) return ECSIMD_HIP_ERR_NO_DEVICE;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) != hipSuccess) return ECSIMD_HIP_ERR_NO_DEVICE;
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) return ECSIMD_HIP_ERR_NO_DEVICE;   // the code object is gfx950-only
  ecsimd_hip_ctx* ctx = new (std::nothrow) ecsimd_hip_ctx();
  if (!ctx) return ECSIMD_HIP_ERR_HIP;
  ctx->device = device; ctx->cus = prop.multiProcessorCount; ctx->err[0] = 0; ctx->sink = nullptr;
  ctx->window_table[0] = ctx->window_table[1] = nullptr; ctx->window6_table[0] = ctx->window6_table[1] = nullptr; ctx->windowct_table[0] = ctx->windowct_table[1] = nullptr; ctx->window16_table[0] = ctx->window16_table[1] = nullptr; ctx->workspace = nullptr; ctx->workspace_bytes = 0; ctx->ref_square = 0; ctx->valid = nullptr; ctx->valid_bytes = 0; ctx->base_special[0] = ctx->base_special[1] = nullptr; ctx->helper = nullptr; ctx->hstage = nullptr; ctx->hstage_bytes = 0;
  ctx->pinned = nullptr; ctx->pinned_bytes = 0; ctx->pinned_copied = nullptr;
  if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&ctx->own_stream, hipStreamNonBlocking) != hipSuccess) { delete ctx; return ECSIMD_HIP_ERR_HIP; }
  ctx->stream = ctx->own_stream;
  if (hipEventCreateWithFlags(&ctx->handoff, hipEventDisableTiming) != hipSuccess) { (void)hipStreamDestroy(ctx->own_stream); delete ctx; return ECSIMD_HIP_ERR_HIP; }
  if (hipMalloc(&ctx->sink, 4096) != hipSuccess) { (void)hipEventDestroy(ctx->handoff); (void)hipStreamDestroy(ctx->own_stream); delete ctx; return ECSIMD_HIP_ERR_HIP; }
  *out = ctx;
  return ECSIMD_HIP_OK;
}
int ecsimd_hip_destroy(ecsimd_hip_ctx* ctx) {
  REQUIRE_CTX();
  (void)hipSetDevice(ctx->device);
  (void)hipStreamSynchronize(ctx->stream);
  (void)hipFree(ctx->sink);
  (void)hipFree(ctx->window_table[0]); (void)hipFree(ctx->window_table[1]); (void)hipFree(ctx->window6_table[0]); (void)hipFree(ctx->window6_table[1]); (void)hipFree(ctx->windowct_table[0]); (void)hipFree(ctx->windowct_table[1]); (void)hipFree(ctx->window16_table[0]); (void)hipFree(ctx->window16_table[1]); (void)hipFree(ctx->workspace); (void)hipFree(ctx->valid); (void)hipFree(ctx->base_special[0]); (void)hipFree(ctx->base_special[1]);
  for (auto& t : ctx->gcomb) { (void)hipFree(t.table); (void)hipFree(t.special); (void)hipFree(t.table7); (void)hipFree(t.table5); (void)hipFree(t.table20); }
  (void)hipFree(ctx->hstage);
  if (ctx->pinned) (void)hipHostFree(ctx->pinned);
  if (ctx->pinned_copied) (void)hipEventDestroy(ctx->pinned_copied);
  if (ctx->helper) (void)ecsimd_hip_destroy(ctx->helper);
  (void)hipEventDestroy(ctx->handoff);
  (void)hipStreamDestroy(ctx->own_stream);
  delete ctx;
  return ECSIMD_HIP_OK;
}
// The context's scratch (workspace, the shared-scalar slot, the lazily built tables) is ordered by its stream.
// Selecting another stream therefore makes that stream wait for what this context already enqueued on the
// previous one (an event, no host synchronisation); re-selecting the current stream costs nothing.
static int switch_stream(ecsimd_hip_ctx* ctx, hipStream_t next) {
  if (next == ctx->stream) return ECSIMD_HIP_OK;
  (void)hipSetDevice(ctx->device);
  // A stream under graph capture can neither wait for an outside event nor lend one: there the caller
  // brackets the capture itself (synchronise before capturing, as graph users do for every library).
  hipStreamCaptureStatus from = hipStreamCaptureStatusNone, to = hipStreamCaptureStatusNone;
  (void)hipStreamIsCapturing(ctx->stream, &from); (void)hipStreamIsCapturing(next, &to);
  (void)hipGetLastError();
  if (from != hipStreamCaptureStatusNone || to != hipStreamCaptureStatusNone) { ctx->stream = next; return ECSIMD_HIP_OK; }
  hipError_t e = hipEventRecord(ctx->handoff, ctx->stream);
  if (e == hipSuccess) e = hipStreamWaitEvent(next, ctx->handoff, 0);
  if (e != hipSuccess) return fail(ctx, e, "stream hand-off");
  ctx->stream = next;
  return ECSIMD_HIP_OK;
}
int ecsimd_hip_set_stream(ecsimd_hip_ctx* ctx, void* s) { REQUIRE_CTX(); return switch_stream(ctx, (hipStream_t)s); }
int ecsimd_hip_use_own_stream(ecsimd_hip_ctx* ctx) { REQUIRE_CTX(); return switch_stream(ctx, ctx->own_stream); }
int ecsimd_hip_set_ref_square_compat(ecsimd_hip_ctx* ctx, int on) { REQUIRE_CTX(); ctx->ref_square = on ? 1 : 0; return ECSIMD_HIP_OK; }
int ecsimd_hip_get_ref_square_compat(const ecsimd_hip_ctx* ctx) { return ctx ? ctx->ref_square : ECSIMD_HIP_ERR_BAD_ARG; }
int ecsimd_hip_sync(ecsimd_hip_ctx* ctx) {
  REQUIRE_CTX();
  REFUSE_IN_CAPTURE("sync waits for the stream");
  hipError_t e = hipStreamSynchronize(ctx->stream);
  return e == hipSuccess ? ECSIMD_HIP_OK : fail(ctx, e, "hipStreamSynchronize");
}
const char* ecsimd_hip_last_error(const ecsimd_hip_ctx* ctx) { return ctx ? ctx->err : "null context"; }
int ecsimd_hip_malloc(ecsimd_hip_ctx* ctx, void** p, size_t bytes) {
  REQUIRE_CTX(); if (!p) return bad(ctx, "dptr is null");
  REFUSE_IN_CAPTURE("malloc allocates device memory");
  (void)hipSetDevice(ctx->device);
  hipError_t e = hipMalloc(p, bytes ? bytes : 16);
  return e == hipSuccess ? ECSIMD_HIP_OK : fail(ctx, e, "hipMalloc");
}
int ecsimd_hip_free(ecsimd_hip_ctx* ctx, void* p) {
  REQUIRE_CTX();
  REFUSE_IN_CAPTURE("free releases device memory, which waits for the device");
  (void)hipSetDevice(ctx->device);
  hipError_t e = hipFree(p);
  return e == hipSuccess ? ECSIMD_HIP_OK : fail(ctx, e, "hipFree");
}
int ecsimd_hip_memcpy_h2d(ecsimd_hip_ctx* ctx, void* dst, const void* src, size_t bytes) {
  REQUIRE_CTX();
  REFUSE_IN_CAPTURE("memcpy_h2d copies from host memory and waits for the copy");
  (void)hipSetDevice(ctx->device);
  hipError_t e = hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);     // src may be pageable: complete before returning
  return e == hipSuccess ? ECSIMD_HIP_OK : fail(ctx, e, "hipMemcpy h2d");
}
int ecsimd_hip_memcpy_d2h(ecsimd_hip_ctx* ctx, void* dst, const void* src, size_t bytes) {
  REQUIRE_CTX();
  REFUSE_IN_CAPTURE("memcpy_d2h copies to host memory and waits for the copy");
  (void)hipSetDevice(ctx->device);
  hipError_t e = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  return e == hipSuccess ? ECSIMD_HIP_OK : fail(ctx, e, "hipMemcpy d2h");
}
int ecsimd_hip_memcpy_d2d(ecsimd_hip_ctx* ctx, void* dst, const void* src, size_t bytes) {
  REQUIRE_CTX(); (void)hipSetDevice(ctx->device);
  if (bytes == 0) return ECSIMD_HIP_OK;
  if (!dst || !src) return bad(ctx, "memcpy_d2d: null pointer");
  hipError_t e = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, ctx->stream);
  return e == hipSuccess ? ECSIMD_HIP_OK : fail(ctx, e, "hipMemcpy d2d");
}


int ecsimd_hip_register_modulus(const uint64_t p[4], int flags, int* field_id) {
  if (!p || !field_id) return ECSIMD_HIP_ERR_BAD_ARG;
  if (!(p[0] & 1u) || (p[0] < 3 && !(p[1] | p[2] | p[3]))) return ECSIMD_HIP_ERR_BAD_ARG;        // odd, >= 3 (Montgomery arithmetic needs gcd(p, 2^256) = 1)
  if (flags & ~ECSIMD_HIP_MODULUS_PRIME) return ECSIMD_HIP_ERR_BAD_ARG;
  // the curve primes keep their special-form kernels
  { uint64_t c[4]; words_to_limbs(curve_consts<CURVE_P256>::P, c); if (!memcmp(c, p, 32)) { *field_id = ECSIMD_HIP_P256; return ECSIMD_HIP_OK; }
    words_to_limbs(curve_consts<CURVE_SECP256K1>::P, c); if (!memcmp(c, p, 32)) { *field_id = ECSIMD_HIP_SECP256K1; return ECSIMD_HIP_OK; } }
  try {
    const gmod M = make_gmod(p, (flags & ECSIMD_HIP_MODULUS_PRIME) ? GMOD_PRIME : 0u);
    modulus_registry& r = registry();
    std::lock_guard<std::mutex> g(r.mu);
    // Entries are keyed on (p, PRIME): the flag changes what gfp_inverse computes (the shared division-step inversion against gfp.h:42-44's x^(p-2), which
    // differ for a composite p), so a registration with the flag must never change the behaviour of an id someone else holds without it.
    for (size_t i = 0; i < r.mods.size(); ++i)
      if (!memcmp(r.mods[i].p, M.p, sizeof M.p) && (r.mods[i].flags == M.flags || i < 2)) { *field_id = FIRST_FIELD_ID + (int)i; return ECSIMD_HIP_OK; }   // (i < 2: the built-in group orders ARE prime, whatever the caller says)
    if (r.mods.size() >= (size_t)MAX_FIELDS) return ECSIMD_HIP_ERR_BAD_ARG;
    r.mods.push_back(M);
    *field_id = FIRST_FIELD_ID + (int)r.mods.size() - 1;
    return ECSIMD_HIP_OK;
  } catch (...) { return ECSIMD_HIP_ERR_BAD_ARG; }             // nothing throws across the C ABI
}

// curve_group<Curve> for any Curve (curve.h:12-15): what the templates derive at compile time, derived here once per curve.
int ecsimd_hip_register_curve(const uint64_t p[4], const uint64_t a[4], const uint64_t b[4], const uint64_t gx[4], const uint64_t gy[4], const uint64_t n[4], int flags, int* curve_id) {
  if (!p || !a || !b || !gx || !gy || !curve_id) return ECSIMD_HIP_ERR_BAD_ARG;
  if (flags & ~ECSIMD_HIP_CURVE_GENERIC_KERNELS) return ECSIMD_HIP_ERR_BAD_ARG;
  const u256 P = u_from(p), A = u_from(a), B = u_from(b), GX = u_from(gx), GY = u_from(gy);
  if ((p[0] & 3u) != 3u || (p[0] < 7 && !(p[1] | p[2] | p[3]))) return ECSIMD_HIP_ERR_BAD_ARG;     // p = 3 mod 4 like the reference's GFp (gfp.h:84), p >= 7
  if (u_geq(A, P) || u_geq(B, P) || u_geq(GX, P) || u_geq(GY, P)) return ECSIMD_HIP_ERR_BAD_ARG;
  // the generator is on the curve (a typo in any of the five values is caught here): y^2 = x^3 + a x + b
  { const u256 lhs = u_mul_mod(GY, GY, P), x3 = u_mul_mod(u_mul_mod(GX, GX, P), GX, P);
    if (!u_eq(lhs, u_add_mod(u_add_mod(x3, u_mul_mod(A, GX, P), P), B, P))) return ECSIMD_HIP_ERR_BAD_ARG; }
  // non-singular: 4 a^3 + 27 b^2 != 0
  { const u256 a3 = u_mul_mod(u_mul_mod(A, A, P), A, P), b2 = u_mul_mod(B, B, P);
    u256 four = {{4, 0, 0, 0}}, c27 = {{27, 0, 0, 0}};
    if (u_geq(four, P)) (void)u_sub(four, four, P);
    while (u_geq(c27, P)) (void)u_sub(c27, c27, P);
    if (u_is_zero(u_add_mod(u_mul_mod(four, a3, P), u_mul_mod(c27, b2, P), P))) return ECSIMD_HIP_ERR_BAD_ARG; }
  u256 N = {{0, 0, 0, 0}};
  if (n) { N = u_from(n); if (!(n[0] & 1u) || u_is_zero(N)) return ECSIMD_HIP_ERR_BAD_ARG; }
  if (!(flags & ECSIMD_HIP_CURVE_GENERIC_KERNELS)) {               // the two built-in curves keep their special-form kernels
    for (int cv = 0; cv < 2; ++cv) {
      uint64_t c[5][4];
      for (int w = 0; w < 5; ++w) (void)ecsimd_hip_get_constant(cv, w, c[w]);
      if (!memcmp(c[0], p, 32) && !memcmp(c[1], a, 32) && !memcmp(c[2], b, 32) && !memcmp(c[3], gx, 32) && !memcmp(c[4], gy, 32)) { *curve_id = cv; return ECSIMD_HIP_OK; }
    }
  }
  try {
    curve_record rec; memset(&rec, 0, sizeof rec);
    rec.a = A; rec.b = B; rec.n = N; rec.has_order = n != nullptr;
    rec.ecdsa_ok = false;
    if (n) {
      // ECDSA on this curve multiplies through the reference's ladder.  For n >= 2^255 the ladder is wrong at n - 1, 2^256 - n - 1 and 2^256 - n alone: such a
      // scalar u is replaced by n - u (k_gc_ladder_safe_scalars).  That needs n - u to be a good scalar in turn; and x mod n by ONE conditional subtraction
      // needs p < 2n.  Below 2^255 every zero bit above the top of u is one more ladder step that can meet infinity: the wrong scalars are then u | 1 = 2^j mod n
      // for every j from n's bit length to 256 (tools/ladder_degenerate_model.py; 2^192 - n and its neighbour on P-192), which that kernel does not know:
      // no ECDSA there.
      rec.N = make_gmod(n, GMOD_PRIME);
      u256 s3[3], alt, twice;
      ladder_degenerate_points(N, s3);
      bool safe = true;
      for (const u256& d : s3) if (!u_geq(d, N)) { (void)u_sub(alt, N, d); if (ladder_degenerate(N, alt)) safe = false; }
      const uint64_t top = N.l[3] >> 63;
      for (int i = 3; i > 0; --i) twice.l[i] = (N.l[i] << 1) | (N.l[i - 1] >> 63);
      twice.l[0] = N.l[0] << 1;
      const bool p_below_2n = top || !u_geq(P, twice);
      rec.ecdsa_ok = safe && p_below_2n && top;
    }
    gcurve& G = rec.G;
    G.F = make_gmod(p, GMOD_PRIME);                                 // registering a CURVE vouches that p is prime
    u_words(G.am, u_shl_mod(A, 256, P));                            // to_mgry(A), to_mgry(B): curve_group.h:31-32
    u_words(G.bm, u_shl_mod(B, 256, P));
    u_words(G.gx, GX); u_words(G.gy, GY);
    u_limbs29(G.r29.p, P);
    G.r29.qinv = G.F.mprime & 0x1fffffffu;                          // -p^-1 mod 2^29 (mprime = -p^-1 mod 2^32)
    const u256 one = {{1, 0, 0, 0}};
    u_limbs29(G.r29.in, u_shl_mod(one, 266, P));                    // 2^266 mod p: x 2^256 -> x 2^261 through one product / 2^261
    u_limbs29(G.r29.out, u_shl_mod(one, 256, P));                   // 2^256 mod p: back
    curve_registry& r = curves();
    auto find = [&]() -> int {
      for (size_t i = 0; i < r.curves.size(); ++i) {
        const curve_record& o = r.curves[i];
        if (!memcmp(o.G.F.p, G.F.p, 32) && u_eq(o.a, A) && u_eq(o.b, B) && !memcmp(o.G.gx, G.gx, 32) && !memcmp(o.G.gy, G.gy, 32) &&
            o.has_order == rec.has_order && (!rec.has_order || u_eq(o.n, N))) return FIRST_CURVE_ID + (int)i;
      }
      return -1;
    };
    { std::lock_guard<std::mutex> g(r.mu); const int id = find(); if (id >= 0) { *curve_id = id; return ECSIMD_HIP_OK; } }
    // A new record only, and outside the registry's lock (~0.1 s of host arithmetic): is n a prime in p's Hasse interval, and then: is it G's order?  One that
    // is not -- a neighbouring prime, a typo -- gets neither the comb nor the window loop nor ECDSA, all of which compute modulo n; the ladder does not.
    rec.prime_order = rec.has_order && (N.l[3] >> 63) != 0 && u_hasse(N, P) && u_probable_prime(N);
    rec.order_wrong = rec.prime_order && !u_order_annihilates(GX, GY, A, P, N);
    if (rec.order_wrong) { rec.prime_order = false; rec.ecdsa_ok = false; }
    std::lock_guard<std::mutex> g(r.mu);
    // Entries are keyed on the curve AND the order it was registered with (none is a value of its own): what an id does -- the small-batch route of
    // scalar_mult_base, the comb, ECDSA -- depends on n, so a later registration with another n (or the first one with any) must never change the
    // behaviour of an id somebody else holds (the rule the modulus registry follows for its PRIME flag).
    { const int id = find(); if (id >= 0) { *curve_id = id; return ECSIMD_HIP_OK; } }                 // (another thread registered the same curve meanwhile)
    if (r.curves.size() >= (size_t)MAX_CURVES) return ECSIMD_HIP_ERR_BAD_ARG;
    r.curves.push_back(rec);
    *curve_id = FIRST_CURVE_ID + (int)r.curves.size() - 1;
    return ECSIMD_HIP_OK;
  } catch (...) { return ECSIMD_HIP_ERR_BAD_ARG; }
}

int ecsimd_hip_curve_capabilities(int curve, int* caps) {
  if (!caps) return ECSIMD_HIP_ERR_BAD_ARG;
  const int all = ECSIMD_HIP_CURVE_HAS_ORDER | ECSIMD_HIP_CURVE_COMB | ECSIMD_HIP_CURVE_ECDSA | ECSIMD_HIP_CURVE_WINDOW_VARIABLE_BASE;
  if (curve == ECSIMD_HIP_P256 || curve == ECSIMD_HIP_SECP256K1) { *caps = all; return ECSIMD_HIP_OK; }
  curve_record rec; if (!lookup_curve_record(curve, &rec)) return ECSIMD_HIP_ERR_BAD_ARG;
  const bool comb = rec.has_order && (rec.n.l[3] >> 63) != 0 && !rec.order_wrong;
  *caps = (rec.has_order ? ECSIMD_HIP_CURVE_HAS_ORDER : 0) | (comb ? ECSIMD_HIP_CURVE_COMB : 0) | (rec.has_order && rec.ecdsa_ok ? ECSIMD_HIP_CURVE_ECDSA : 0) |
          (comb && rec.prime_order ? ECSIMD_HIP_CURVE_WINDOW_VARIABLE_BASE : 0);
  return ECSIMD_HIP_OK;
}

int ecsimd_hip_get_constant(int curve, int which, uint64_t out[4]) {
  if (!out || which < 0 || which > 11) return ECSIMD_HIP_ERR_BAD_ARG;
#define PICK(C) do { using K = curve_consts<C>; using E = curve_exps<C>; \
    switch (which) { \
      case 0: words_to_limbs(K::P, out); break; \
      case 1: { uint32_t a[8]; for (int i = 0; i < 8; ++i) a[i] = (C == CURVE_P256) ? K::P[i] : 0u; if (C == CURVE_P256) a[0] -= 3u; words_to_limbs(a, out); break; } \
      case 2: { static const uint32_t b256[8] = {0x27d2604bu, 0x3bce3c3eu, 0xcc53b0f6u, 0x651d06b0u, 0x769886bcu, 0xb3ebbd55u, 0xaa3a93e7u, 0x5ac635d8u}; \
                static const uint32_t bk1[8] = {7u, 0, 0, 0, 0, 0, 0, 0}; words_to_limbs((C == CURVE_P256) ? b256 : bk1, out); break; } \
      case 3: words_to_limbs(K::GX, out); break; \
      case 4: words_to_limbs(K::GY, out); break; \
      case 5: words_to_limbs(K::R_P, out); break; \
      case 6: words_to_limbs(K::RSQ, out); break; \
      case 7: { /* -R mod p = p - (R mod p) */ uint64_t p[4], r[4]; words_to_limbs(K::P, p); words_to_limbs(K::R_P, r); \
                unsigned __int128 bw = 0; for (int i = 0; i < 4; ++i) { unsigned __int128 d = (unsigned __int128)p[i] - r[i] - (uint64_t)bw; out[i] = (uint64_t)d; bw = (d >> 64) & 1; } break; } \
      case 8: words_to_limbs(K::AM, out); break; \
      case 9: words_to_limbs(K::BM, out); break; \
      case 10: words_to_limbs(E::P_M2, out); break; \
      default: words_to_limbs(E::P_SQRT, out); break; \
    } } while (0)
  if (curve == ECSIMD_HIP_P256) PICK(CURVE_P256);
  else if (curve == ECSIMD_HIP_SECP256K1) PICK(CURVE_SECP256K1);
  else {
    // a registered curve: every slot
    curve_record rec;
    if (lookup_curve_record(curve, &rec)) {
      switch (which) {
        case 1: memcpy(out, rec.a.l, 32); return ECSIMD_HIP_OK;
        case 2: memcpy(out, rec.b.l, 32); return ECSIMD_HIP_OK;
        case 3: words_to_limbs(rec.G.gx, out); return ECSIMD_HIP_OK;
        case 4: words_to_limbs(rec.G.gy, out); return ECSIMD_HIP_OK;
        case 8: words_to_limbs(rec.G.am, out); return ECSIMD_HIP_OK;
        case 9: words_to_limbs(rec.G.bm, out); return ECSIMD_HIP_OK;
        default: break;                                    // the field's slots below
      }
    }
    // a field id: p, R mod p, R^2 mod p, -R mod p, p - 2, (p + 1) / 4; the curve slots (a, b, Gx, Gy, a R, b R) read zero
    gmod M;
    if (!lookup_modulus(curve, &M)) return ECSIMD_HIP_ERR_BAD_ARG;
    static const uint32_t zero[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    switch (which) {
      case 0: words_to_limbs(M.p, out); break;
      case 5: words_to_limbs(M.r, out); break;
      case 6: words_to_limbs(M.rsq, out); break;
      case 7: words_to_limbs(M.negr, out); break;
      case 10: words_to_limbs(M.pm2, out); break;
      case 11: words_to_limbs(M.psqrt, out); break;
      default: words_to_limbs(zero, out); break;
    }
  }
#undef PICK
  return ECSIMD_HIP_OK;
}

// ---- L2
int ecsimd_hip_add(ecsimd_hip_ctx* ctx, const uint64_t* a, const uint64_t* b, uint64_t* out, uint8_t* carry, size_t n) {
  REQUIRE_CTX(); REQUIRE_PTR(a); REQUIRE_PTR(b); REQUIRE_PTR(out); RUN(launch::add(s, a, b, out, carry, n)); }
int ecsimd_hip_sub(ecsimd_hip_ctx* ctx, const uint64_t* a, const uint64_t* b, uint64_t* out, uint8_t* borrow, size_t n) {
  REQUIRE_CTX(); REQUIRE_PTR(a); REQUIRE_PTR(b); REQUIRE_PTR(out); RUN(launch::sub(s, a, b, out, borrow, n)); }
int ecsimd_hip_sub_if_above(ecsimd_hip_ctx* ctx, const uint64_t* a, const uint64_t* p, uint64_t* out, size_t n) {
  REQUIRE_CTX(); REQUIRE_PTR(a); REQUIRE_PTR(p); REQUIRE_PTR(out); RUN(launch::sub_if_above(s, a, p, out, n)); }
int ecsimd_hip_cmp_lt(ecsimd_hip_ctx* ctx, const uint64_t* a, const uint64_t* b, uint8_t* flag, size_t n) {
  REQUIRE_CTX(); REQUIRE_PTR(a); REQUIRE_PTR(b); if (!flag && n) return bad(ctx, "flag is null");
  RUN(launch::sub(s, a, b, nullptr, flag, n)); }
int ecsimd_hip_cmp_eq(ecsimd_hip_ctx* ctx, const uint64_t* a, const uint64_t* b, int limbs, uint8_t* flag, size_t n) {
  REQUIRE_CTX(); REQUIRE_PTR(a); REQUIRE_PTR(b); if (!flag && n) return bad(ctx, "flag is null");
  if (limbs < 1 || limbs > 8) return bad(ctx, "limbs must be 1..8");
  RUN(launch::cmp_eq(s, a, b, limbs, flag, n)); }
int ecsimd_hip_mask_op(ecsimd_hip_ctx* ctx, int op, const uint8_t* a, const uint8_t* b, uint8_t* out, size_t n) {
  REQUIRE_CTX(); if (op < ECSIMD_HIP_MASK_NOT || op > ECSIMD_HIP_MASK_EQ) return bad(ctx, "unknown mask operation");
  if (n && (!a || !out || (op != ECSIMD_HIP_MASK_NOT && !b))) return bad(ctx, "mask pointer is null");
  RUN(launch::mask_op(s, op, a, b, out, n)); }
int ecsimd_hip_mask_count(ecsimd_hip_ctx* ctx, const uint8_t* a, size_t n, size_t* count) {
  REQUIRE_CTX(); if (!count) return bad(ctx, "count is null");
  *count = 0;
  if (!a && n) return bad(ctx, "mask pointer is null");
  REFUSE_IN_CAPTURE("mask_count returns the count to the host");      // before the empty batch's early return: one answer whatever n is
  ENTER_ANY_SIZE();
  unsigned long long* slot = reinterpret_cast<unsigned long long*>(ctx->sink + 1024 - 16);     // 8-byte slot next to the shared scalar
  hipError_t e = hipMemsetAsync(slot, 0, sizeof *slot, ctx->stream);
  if (e == hipSuccess) { launch::mask_count(ctx->stream, a, n, slot); e = hipGetLastError(); }
  unsigned long long host = 0;
  if (e == hipSuccess) e = hipMemcpyAsync(&host, slot, sizeof host, hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) return fail(ctx, e, "mask_count");
  *count = (size_t)host;
  return ECSIMD_HIP_OK; }
int ecsimd_hip_shift_left_one(ecsimd_hip_ctx* ctx, const uint64_t* a, uint64_t* out, uint8_t* carry, size_t n) {
  REQUIRE_CTX(); REQUIRE_PTR(a); REQUIRE_PTR(out); RUN(launch::shift_left_one(s, a, out, carry, n)); }
int ecsimd_hip_mul(ecsimd_hip_ctx* ctx, const uint64_t* a, const uint64_t* b, uint64_t* out8, size_t n) {
  REQUIRE_CTX(); REQUIRE_PTR(a); REQUIRE_PTR(b); REQUIRE_PTR(out8); RUN(launch::mul(s, a, b, out8, n)); }
int ecsimd_hip_square(ecsimd_hip_ctx* ctx, const uint64_t* a, uint64_t* out8, size_t n) {
  REQUIRE_CTX(); REQUIRE_PTR(a); REQUIRE_PTR(out8); RUN(launch::square(s, a, out8, n, ctx->ref_square != 0)); }
int ecsimd_hip_swap_if(ecsimd_hip_ctx* ctx, const uint8_t* mask, uint64_t* a, uint64_t* b, size_t n) {
  REQUIRE_CTX(); REQUIRE_PTR(a); REQUIRE_PTR(b); if (!mask && n) return bad(ctx, "mask is null"); RUN(launch::swap_if(s, mask, a, b, n)); }
int ecsimd_hip_if_else(ecsimd_hip_ctx* ctx, const uint8_t* mask, const uint64_t* a, const uint64_t* b, uint64_t* out, size_t n) {
  REQUIRE_CTX(); REQUIRE_PTR(a); REQUIRE_PTR(b); REQUIRE_PTR(out); if (!mask && n) return bad(ctx, "mask is null"); RUN(launch::if_else(s, mask, a, b, out, n)); }

// ---- wire formats
int ecsimd_hip_from_bytes_be(ecsimd_hip_ctx* ctx, const uint8_t* bytes, uint64_t* out, size_t n) {
  REQUIRE_CTX(); REQUIRE_PTR(bytes); REQUIRE_PTR(out); RUN(launch::bytes_be(s, bytes, out, n)); }
int ecsimd_hip_to_bytes_be(ecsimd_hip_ctx* ctx, const uint64_t* in, uint8_t* bytes, size_t n) {
  REQUIRE_CTX(); REQUIRE_PTR(in); REQUIRE_PTR(bytes); RUN(launch::bytes_be(s, in, bytes, n)); }
// The reference's register layout (four lanes per wide, limb-major: bignum.h:99-100) <-> the ABI's one element per lane, on the device.
int ecsimd_hip_wide4_to_lanes(ecsimd_hip_ctx* ctx, const void* wides, size_t record_bytes, size_t offset_bytes, uint64_t* out, size_t n_wides) {
  REQUIRE_CTX(); const size_t n = 4 * n_wides; REQUIRE_PTR(out); if (!wides && n) return bad(ctx, "wides is null");
  if (static_cast<const void*>(out) == wides) return bad(ctx, "the transposition is not in place: out must not alias wides");
  if (record_bytes < 128 || (record_bytes & 7u) || (offset_bytes & 7u) || offset_bytes + 128 > record_bytes || (reinterpret_cast<uintptr_t>(wides) & 7u)) return bad(ctx, "a wide is 128 bytes at an 8-byte aligned offset inside its record");
  if (n_wides > MAX_LAUNCH / 4) return bad(ctx, "batch too large");
  RUN(launch::wide4_to_lanes(s, wides, record_bytes, offset_bytes, out, n)); }
int ecsimd_hip_lanes_to_wide4(ecsimd_hip_ctx* ctx, const uint64_t* in, void* wides, size_t record_bytes, size_t offset_bytes, size_t n_wides) {
  REQUIRE_CTX(); const size_t n = 4 * n_wides; REQUIRE_PTR(in); if (!wides && n) return bad(ctx, "wides is null");
  if (static_cast<const void*>(in) == wides) return bad(ctx, "the transposition is not in place: wides must not alias in");
  if (record_bytes < 128 || (record_bytes & 7u) || (offset_bytes & 7u) || offset_bytes + 128 > record_bytes || (reinterpret_cast<uintptr_t>(wides) & 7u)) return bad(ctx, "a wide is 128 bytes at an 8-byte aligned offset inside its record");
  if (n_wides > MAX_LAUNCH / 4) return bad(ctx, "batch too large");
  RUN(launch::lanes_to_wide4(s, in, wides, record_bytes, offset_bytes, n)); }
int ecsimd_hip_mask_bit(ecsimd_hip_ctx* ctx, const uint64_t* a, int bit, uint8_t* flag, size_t n) {
  REQUIRE_CTX(); REQUIRE_PTR(a); if (!flag && n) return bad(ctx, "flag is null"); if (bit < 0 || bit > 255) return bad(ctx, "bit index");
  RUN(launch::mask_bit(s, a, bit, flag, n)); }
int ecsimd_hip_sec1_encode(ecsimd_hip_ctx* ctx, int curve, const uint64_t* x, const uint64_t* y, uint8_t* out, size_t n, int compressed) {
  REQUIRE_CTX(); REQUIRE_PTR(x); REQUIRE_PTR(y); REQUIRE_PTR(out);
  if (curve >= ECSIMD_HIP_FIRST_REGISTERED_CURVE) { gcurve GC; if (!lookup_curve(curve, &GC)) return bad(ctx, "unknown curve id"); curve = ECSIMD_HIP_P256; }     // the encoding does not look at the curve
  REQUIRE_CURVE(); RUN(launch::sec1_encode(s, curve, x, y, out, n, compressed != 0)); }
int ecsimd_hip_sec1_decode(ecsimd_hip_ctx* ctx, int curve, const uint8_t* in, uint64_t* x, uint64_t* y, uint8_t* ok, size_t n, int compressed) {
  REQUIRE_CTX(); REQUIRE_PTR(in); REQUIRE_PTR(x); REQUIRE_PTR(y); GENERIC_CURVE(launch::gc_sec1_decode(s, GC, in, x, y, ok, n, compressed != 0));
  REQUIRE_CURVE(); RUN(launch::sec1_decode(s, curve, in, x, y, ok, n, compressed != 0)); }

// ---- L3.  `curve` is a FIELD id here: a curve's prime (0, 1: the special-form kernels of field.cuh) or a run-time modulus (>= 2: k_gfield.hip).
#define FIELD_OR_CURVE(generic_call) do { if (curve != ECSIMD_HIP_P256 && curve != ECSIMD_HIP_SECP256K1) { \
    gmod M; if (!lookup_modulus(curve, &M)) return bad(ctx, "unknown curve / field id"); RUN(generic_call); } } while (0)
int ecsimd_hip_mod_add(ecsimd_hip_ctx* ctx, int curve, const uint64_t* a, const uint64_t* b, uint64_t* out, size_t n) {
  REQUIRE_CTX(); REQUIRE_PTR(a); REQUIRE_PTR(b); REQUIRE_PTR(out); FIELD_OR_CURVE(launch::gfield_binop(s, M, launch::F_MOD_ADD, a, b, out, n)); RUN(launch::field_binop(s, instance(ctx, curve), launch::F_MOD_ADD, a, b, out, n)); }
int ecsimd_hip_mod_sub(ecsimd_hip_ctx* ctx, int curve, const uint64_t* a, const uint64_t* b, uint64_t* out, size_t n) {
  REQUIRE_CTX(); REQUIRE_PTR(a); REQUIRE_PTR(b); REQUIRE_PTR(out); FIELD_OR_CURVE(launch::gfield_binop(s, M, launch::F_MOD_SUB, a, b, out, n)); RUN(launch::field_binop(s, instance(ctx, curve), launch::F_MOD_SUB, a, b, out, n)); }
int ecsimd_hip_mod_mul(ecsimd_hip_ctx* ctx, int curve, const uint64_t* a, const uint64_t* b, uint64_t* out, size_t n) {
  REQUIRE_CTX(); REQUIRE_PTR(a); REQUIRE_PTR(b); REQUIRE_PTR(out); FIELD_OR_CURVE(launch::gfield_mod_mul(s, M, a, b, out, n)); RUN(launch::mod_mul(s, instance(ctx, curve), a, b, out, n)); }
int ecsimd_hip_mod_shift_left(ecsimd_hip_ctx* ctx, int curve, const uint64_t* a, int count, uint64_t* out, size_t n) {
  REQUIRE_CTX(); REQUIRE_PTR(a); REQUIRE_PTR(out); if ((count & 0xff) < 1 || (count & ~0x1ff)) return bad(ctx, "count must be 1..255, optionally | ECSIMD_HIP_SHIFT_FUSED"); FIELD_OR_CURVE(launch::gfield_shift_left(s, M, a, count, out, n)); RUN(launch::mod_shift_left(s, instance(ctx, curve), a, count, out, n)); }
int ecsimd_hip_mgry_reduce(ecsimd_hip_ctx* ctx, int curve, const uint64_t* a8, uint64_t* out, size_t n) {
  REQUIRE_CTX(); REQUIRE_PTR(a8); REQUIRE_PTR(out); FIELD_OR_CURVE(launch::gfield_reduce(s, M, a8, out, n)); RUN(launch::mgry_reduce(s, instance(ctx, curve), a8, out, n)); }
int ecsimd_hip_mgry_mul(ecsimd_hip_ctx* ctx, int curve, const uint64_t* a, const uint64_t* b, uint64_t* out, size_t n) {
  REQUIRE_CTX(); REQUIRE_PTR(a); REQUIRE_PTR(b); REQUIRE_PTR(out); FIELD_OR_CURVE(launch::gfield_binop(s, M, launch::F_MGRY_MUL, a, b, out, n)); RUN(launch::field_binop(s, instance(ctx, curve), launch::F_MGRY_MUL, a, b, out, n)); }
int ecsimd_hip_mgry_sqr(ecsimd_hip_ctx* ctx, int curve, const uint64_t* a, uint64_t* out, size_t n) {
  REQUIRE_CTX(); REQUIRE_PTR(a); REQUIRE_PTR(out); FIELD_OR_CURVE(launch::gfield_unop(s, M, launch::F_MGRY_SQR, a, out, n, ctx->ref_square != 0)); RUN(launch::field_unop(s, instance(ctx, curve), launch::F_MGRY_SQR, a, out, n)); }
int ecsimd_hip_mgry_from_classical(ecsimd_hip_ctx* ctx, int curve, const uint64_t* a, uint64_t* out, size_t n) {
  REQUIRE_CTX(); REQUIRE_PTR(a); REQUIRE_PTR(out); FIELD_OR_CURVE(launch::gfield_unop(s, M, launch::F_FROM_CLASSICAL, a, out, n, false)); RUN(launch::field_unop(s, instance(ctx, curve), launch::F_FROM_CLASSICAL, a, out, n)); }
int ecsimd_hip_mgry_to_classical(ecsimd_hip_ctx* ctx, int curve, const uint64_t* a, uint64_t* out, size_t n) {
  REQUIRE_CTX(); REQUIRE_PTR(a); REQUIRE_PTR(out); FIELD_OR_CURVE(launch::gfield_unop(s, M, launch::F_TO_CLASSICAL, a, out, n, false)); RUN(launch::field_unop(s, instance(ctx, curve), launch::F_TO_CLASSICAL, a, out, n)); }
int ecsimd_hip_mgry_pow(ecsimd_hip_ctx* ctx, int curve, const uint64_t* a, const uint64_t exponent[4], uint64_t* out, size_t n) {
  REQUIRE_CTX(); REQUIRE_PTR(a); REQUIRE_PTR(out); if (!exponent) return bad(ctx, "exponent is null");
  const launch::words8 e = words8_of(exponent);
  FIELD_OR_CURVE(launch::gfield_pow(s, M, a, e, out, n, ctx->ref_square != 0));
  RUN(launch::mgry_pow(s, instance(ctx, curve), a, e, out, n)); }
int ecsimd_hip_gfp_inverse(ecsimd_hip_ctx* ctx, int curve, const uint64_t* a, uint64_t* out, size_t n) {
  REQUIRE_CTX(); REQUIRE_PTR(a); REQUIRE_PTR(out);
  if (curve != ECSIMD_HIP_P256 && curve != ECSIMD_HIP_SECP256K1) {
    // a run-time modulus.  Registered as PRIME: the shared division-step inversion below (the unique inverse = x^(p-2)); otherwise x^(p-2) bit by
    // bit, which is what gfp.h:42-44 computes whatever p is (for a composite p it is not an inverse, and the reference returns it all the same).
    gmod M; if (!lookup_modulus(curve, &M)) return bad(ctx, "unknown curve / field id");
    if ((M.flags & GMOD_PRIME) && !ctx->ref_square && !overlaps(out, a)) RUN(launch::gfield_inverse_batched(s, M, a, out, n));
    RUN(launch::gfield_unop(s, M, launch::F_INVERSE, a, out, n, ctx->ref_square != 0));
  }
  // one inversion per ~64 elements (Montgomery's trick, out[] as scratch) unless the call is in place
  // (the reference-square instances raise to p - 2 per element, squaring by squaring as the reference does)
  if (overlaps(out, a) || ctx->ref_square) RUN(launch::field_unop(s, instance(ctx, curve), launch::F_INVERSE, a, out, n));
  RUN(launch::inverse_batched(s, curve, a, out, n)); }
int ecsimd_hip_gfp_opposite(ecsimd_hip_ctx* ctx, int curve, const uint64_t* a, uint64_t* out, size_t n) {
  REQUIRE_CTX(); REQUIRE_PTR(a); REQUIRE_PTR(out); FIELD_OR_CURVE(launch::gfield_unop(s, M, launch::F_OPPOSITE, a, out, n, false)); RUN(launch::field_unop(s, instance(ctx, curve), launch::F_OPPOSITE, a, out, n)); }
int ecsimd_hip_gfp_sqrt(ecsimd_hip_ctx* ctx, int curve, const uint64_t* a, uint64_t* out, uint8_t* ok, size_t n) {
  REQUIRE_CTX(); REQUIRE_PTR(a); REQUIRE_PTR(out);
  if (curve != ECSIMD_HIP_P256 && curve != ECSIMD_HIP_SECP256K1) {
    gmod M; if (!lookup_modulus(curve, &M)) return bad(ctx, "unknown curve / field id");
    if (!(M.flags & GMOD_3MOD4)) return bad(ctx, "gfp_sqrt needs p = 3 mod 4 (the reference's GFp does not instantiate otherwise: gfp.h:84)");
    RUN(launch::gfield_sqrt(s, M, a, out, ok, n, ctx->ref_square != 0));
  }
  RUN(launch::gfp_sqrt(s, instance(ctx, curve), a, out, ok, n)); }

// ---- L4/L5
int ecsimd_hip_from_affine(ecsimd_hip_ctx* ctx, int curve, const uint64_t* x, const uint64_t* y, uint64_t* jx, uint64_t* jy, uint64_t* jz, size_t n) {
  REQUIRE_CTX(); REQUIRE_PTR(x); REQUIRE_PTR(y); REQUIRE_PTR(jx); REQUIRE_PTR(jy); REQUIRE_PTR(jz); GENERIC_CURVE(launch::gc_from_affine(s, GC, x, y, jx, jy, jz, n));
  REQUIRE_CURVE(); RUN(launch::from_affine(s, instance(ctx, curve), x, y, jx, jy, jz, n)); }
int ecsimd_hip_to_affine(ecsimd_hip_ctx* ctx, int curve, const uint64_t* jx, const uint64_t* jy, const uint64_t* jz, uint64_t* x, uint64_t* y, size_t n) {
  REQUIRE_CTX(); REQUIRE_PTR(jx); REQUIRE_PTR(jy); REQUIRE_PTR(jz); REQUIRE_PTR(x);
  if (y && !aligned16(y)) return bad(ctx, "y is not 16-byte aligned");       // y == NULL: the x coordinate only
  // Simultaneous inversion uses x[] as scratch: only when the outputs do not alias the inputs.
  const bool alias = any_alias({x, y}, {jx, jy, jz});
  if (alias || ctx->ref_square) GENERIC_CURVE(launch::gc_to_affine(s, GC, jx, jy, jz, x, y, n, ctx->ref_square != 0));
  GENERIC_CURVE(launch::gc_to_affine_batched(s, GC, jx, jy, jz, x, y, n));
  REQUIRE_CURVE();
  if (alias || ctx->ref_square) RUN(launch::to_affine(s, instance(ctx, curve), jx, jy, jz, x, y, n));
  RUN(launch::to_affine_batched(s, curve, jx, jy, jz, x, y, n, false)); }
int ecsimd_hip_compute_y(ecsimd_hip_ctx* ctx, int curve, const uint64_t* x, uint64_t* y, uint8_t* ok, size_t n) {
  REQUIRE_CTX(); REQUIRE_PTR(x); REQUIRE_PTR(y); GENERIC_CURVE(launch::gc_compute_y(s, GC, x, y, ok, n, ctx->ref_square != 0));
  REQUIRE_CURVE(); RUN(launch::compute_y(s, instance(ctx, curve), x, y, ok, n)); }
int ecsimd_hip_dblu(ecsimd_hip_ctx* ctx, int curve, uint64_t* px, uint64_t* py, uint64_t* pz, uint64_t* rx, uint64_t* ry, uint64_t* rz, size_t n) {
  REQUIRE_CTX(); REQUIRE_PTR(px); REQUIRE_PTR(py); REQUIRE_PTR(pz); REQUIRE_PTR(rx); REQUIRE_PTR(ry); REQUIRE_PTR(rz); GENERIC_CURVE(launch::gc_dblu(s, GC, px, py, pz, rx, ry, rz, n, ctx->ref_square != 0));
  REQUIRE_CURVE(); RUN(launch::dblu(s, instance(ctx, curve), px, py, pz, rx, ry, rz, n)); }
int ecsimd_hip_zaddu(ecsimd_hip_ctx* ctx, int curve, uint64_t* px, uint64_t* py, uint64_t* pz, const uint64_t* ox, const uint64_t* oy, const uint64_t* oz, uint64_t* rx, uint64_t* ry, uint64_t* rz, size_t n) {
  REQUIRE_CTX(); REQUIRE_PTR(px); REQUIRE_PTR(py); REQUIRE_PTR(pz); REQUIRE_PTR(ox); REQUIRE_PTR(oy); REQUIRE_PTR(rx); REQUIRE_PTR(ry); REQUIRE_PTR(rz);
  (void)oz;   // co-Z: O.z == P.z by precondition (curve_group.h:92)
  GENERIC_CURVE(launch::gc_zaddu(s, GC, px, py, pz, ox, oy, rx, ry, rz, n, ctx->ref_square != 0));
  REQUIRE_CURVE(); RUN(launch::zaddu(s, instance(ctx, curve), px, py, pz, ox, oy, rx, ry, rz, n)); }
int ecsimd_hip_zdau(ecsimd_hip_ctx* ctx, int curve, const uint64_t* px, const uint64_t* py, const uint64_t* pz, uint64_t* qx, uint64_t* qy, uint64_t* qz, uint64_t* rx, uint64_t* ry, uint64_t* rz, size_t n) {
  REQUIRE_CTX(); REQUIRE_PTR(px); REQUIRE_PTR(py); REQUIRE_PTR(pz); REQUIRE_PTR(qx); REQUIRE_PTR(qy); REQUIRE_PTR(qz); REQUIRE_PTR(rx); REQUIRE_PTR(ry); REQUIRE_PTR(rz);
  GENERIC_CURVE(launch::gc_zdau(s, GC, px, py, pz, qx, qy, qz, rx, ry, rz, n, ctx->ref_square != 0));
  REQUIRE_CURVE(); RUN(launch::zdau(s, instance(ctx, curve), px, py, pz, qx, qy, qz, rx, ry, rz, n)); }
int ecsimd_hip_zdau_repeat(ecsimd_hip_ctx* ctx, int curve, const uint64_t* px, const uint64_t* py, const uint64_t* pz, const uint64_t* qx, const uint64_t* qy,
                           uint64_t* rx, uint64_t* ry, uint64_t* sx, uint64_t* sy, uint64_t* oz, size_t n, int iters, uint64_t swap_bits, int radix) {
  REQUIRE_CTX(); REQUIRE_PTR(px); REQUIRE_PTR(py); REQUIRE_PTR(pz); REQUIRE_PTR(qx); REQUIRE_PTR(qy); REQUIRE_PTR(rx); REQUIRE_PTR(ry); REQUIRE_PTR(sx); REQUIRE_PTR(sy); REQUIRE_PTR(oz);
  if (iters < 0) return bad(ctx, "iters is negative");
  if (radix != 29 && radix != 32) return bad(ctx, "radix is 29 or 32");
  if (curve >= ECSIMD_HIP_FIRST_REGISTERED_CURVE && ctx->ref_square) return bad(ctx, "zdau_repeat on a registered curve has no reference-square form");
  GENERIC_CURVE(launch::gc_zdau_repeat(s, GC, px, py, pz, qx, qy, rx, ry, sx, sy, oz, n, iters, swap_bits, radix));
  REQUIRE_CURVE();
  if (radix == 29 && instance(ctx, curve) != curve) return bad(ctx, "the reduced-radix loop has no reference-square form (the dropped carry depends on the 32-bit Montgomery digits)");
  RUN(launch::zdau_repeat(s, instance(ctx, curve), px, py, pz, qx, qy, rx, ry, sx, sy, oz, n, iters, swap_bits, radix)); }
int ecsimd_hip_add_z2_1(ecsimd_hip_ctx* ctx, int curve, const uint64_t* ax, const uint64_t* ay, const uint64_t* az, const uint64_t* bx, const uint64_t* by, uint64_t* rx, uint64_t* ry, uint64_t* rz, size_t n) {
  REQUIRE_CTX(); REQUIRE_PTR(ax); REQUIRE_PTR(ay); REQUIRE_PTR(az); REQUIRE_PTR(bx); REQUIRE_PTR(by); REQUIRE_PTR(rx); REQUIRE_PTR(ry); REQUIRE_PTR(rz);
  GENERIC_CURVE(launch::gc_add_z2_1(s, GC, ax, ay, az, bx, by, rx, ry, rz, n, ctx->ref_square != 0));
  REQUIRE_CURVE(); RUN(launch::add_z2_1(s, instance(ctx, curve), ax, ay, az, bx, by, rx, ry, rz, n)); }
int ecsimd_hip_add_mixed_complete(ecsimd_hip_ctx* ctx, int curve, const uint64_t* ax, const uint64_t* ay, const uint64_t* az, const uint64_t* bx, const uint64_t* by, uint64_t* rx, uint64_t* ry, uint64_t* rz, size_t n) {
  REQUIRE_CTX(); REQUIRE_CURVE(); REQUIRE_PTR(ax); REQUIRE_PTR(ay); REQUIRE_PTR(az); REQUIRE_PTR(bx); REQUIRE_PTR(by); REQUIRE_PTR(rx); REQUIRE_PTR(ry); REQUIRE_PTR(rz);
  RUN(launch::add_mixed_complete(s, curve, ax, ay, az, bx, by, rx, ry, rz, n)); }
int ecsimd_hip_trplu(ecsimd_hip_ctx* ctx, int curve, uint64_t* px, uint64_t* py, uint64_t* pz, uint64_t* rx, uint64_t* ry, uint64_t* rz, size_t n) {
  REQUIRE_CTX(); REQUIRE_PTR(px); REQUIRE_PTR(py); REQUIRE_PTR(pz); REQUIRE_PTR(rx); REQUIRE_PTR(ry); REQUIRE_PTR(rz); GENERIC_CURVE(launch::gc_trplu(s, GC, px, py, pz, rx, ry, rz, n, ctx->ref_square != 0));
  REQUIRE_CURVE(); RUN(launch::trplu(s, instance(ctx, curve), px, py, pz, rx, ry, rz, n)); }

// scalar_mult and scalar_mult_1s behind their argument checks: k_stride = 4 (a scalar per lane) or 0 (one for all).
static int variable_base_mult(ecsimd_hip_ctx* ctx, int curve, const uint64_t* k, int k_stride, const uint64_t* x, const uint64_t* y, uint64_t* ox, uint64_t* oy, uint64_t* oz, size_t n, int flags) {
  if (curve >= ECSIMD_HIP_FIRST_REGISTERED_CURVE) return run_gladder(ctx, curve, k, k_stride, x, y, ox, oy, oz, n, flags);
  REQUIRE_CURVE();
  if (flags & (ECSIMD_HIP_ALG_WINDOWED | ECSIMD_HIP_ALG_WINDOWED_SIGNED)) {
    // per-lane window tables (8 multiples of P) in HBM + signed 4-bit windows (k_varwin.inc): a different algorithm from
    // the reference ladder, so affine output only (SURVEY.md 8(a) level A)
    if (!(flags & ECSIMD_HIP_OUT_AFFINE)) return bad(ctx, "ALG_WINDOWED needs OUT_AFFINE");
    if ((flags & ECSIMD_HIP_ALG_CONSTANT_TIME) && (flags & ECSIMD_HIP_ALG_WINDOWED_SIGNED)) return bad(ctx, "ALG_CONSTANT_TIME modifies ALG_WINDOWED only, not ALG_WINDOWED_SIGNED");
    NO_COMPAT("ALG_WINDOWED");
    return run_varwin(ctx, curve, k, k_stride, x, y, ox, oy, n, flags, 0);
  }
  if (flags & ECSIMD_HIP_ALG_CONSTANT_TIME) return bad(ctx, "ALG_CONSTANT_TIME modifies ALG_WINDOWED (the ladder is constant-time as it is)");
  return run_ladder(ctx, curve, k, k_stride, x, y, ox, oy, oz, n, flags);
}

int ecsimd_hip_scalar_mult(ecsimd_hip_ctx* ctx, int curve, const uint64_t* k, const uint64_t* x, const uint64_t* y, uint64_t* ox, uint64_t* oy, uint64_t* oz, size_t n, int flags) {
  REQUIRE_CTX();
  // no base point AND the caller says so (BASE_GENERATOR): the generator.  Two null pointers alone are an error, as they were before round 4 -- a caller whose
  // point buffers failed to allocate must not get k G back (and ALG_WINDOWED means another algorithm on a fixed base than on a variable one).
  if ((flags & ECSIMD_HIP_BASE_GENERATOR) && x == nullptr && y == nullptr)
    return ecsimd_hip_scalar_mult_base(ctx, curve, k, ox, oy, oz, n, flags & ~(ECSIMD_HIP_BASE_MGRY | ECSIMD_HIP_BASE_GENERATOR));
  if (flags & ECSIMD_HIP_BASE_GENERATOR) return bad(ctx, "BASE_GENERATOR takes x = y = NULL");
  REQUIRE_PTR(k); REQUIRE_PTR(x); REQUIRE_PTR(y); REQUIRE_PTR(ox); REQUIRE_OUT_Y(oy);
  if (!(flags & ECSIMD_HIP_OUT_AFFINE)) REQUIRE_PTR(oz);
  return variable_base_mult(ctx, curve, k, 4, x, y, ox, oy, oz, n, flags); }
// ---- host arrays in, host arrays out: the PCIe-inclusive form of scalar_mult.  Chunks of 2^19 elements alternate between this context and a helper context (a
// second HIP stream): while the ladder of one chunk runs, the calling thread copies the next chunk in on the other side and launches it, then waits for the
// previous chunk and copies it out -- the copies of one chunk overlap the ladder of its neighbour and the GPU always has a launch queued; the caller's arrays
// may be ordinary pageable memory.  Synchronous: returns with the results in place.
namespace {
constexpr size_t HOST_CHUNK = (size_t)1 << 19;
struct host_side { ecsimd_hip_ctx* c; uint64_t *k, *x, *y, *o[3]; };
int host_stage(ecsimd_hip_ctx* c, size_t elems, int arrays, host_side* S) {
  const size_t bytes = (size_t)arrays * elems * 32;
  if (c->hstage_bytes < bytes) {
    (void)hipStreamSynchronize(c->stream);
    (void)hipFree(c->hstage); c->hstage = nullptr; c->hstage_bytes = 0;
    hipError_t e = hipMalloc(&c->hstage, bytes);
    if (e != hipSuccess) return fail(c, e, "scalar_mult_host staging");
    c->hstage_bytes = bytes;
  }
  uint64_t* p = c->hstage;
  S->c = c; S->k = p; S->x = p + 4 * elems; S->y = p + 8 * elems;
  for (int j = 0; j < 3; ++j) S->o[j] = p + (size_t)(3 + j) * 4 * elems;
  return ECSIMD_HIP_OK;
}
}  // namespace
int ecsimd_hip_scalar_mult_host(ecsimd_hip_ctx* ctx, int curve, const uint64_t* k, const uint64_t* x, const uint64_t* y, uint64_t* ox, uint64_t* oy, uint64_t* oz, size_t n, int flags) {
  REQUIRE_CTX();
  const bool generator = (flags & ECSIMD_HIP_BASE_GENERATOR) != 0, affine = (flags & ECSIMD_HIP_OUT_AFFINE) != 0;
  if (!k || !ox) return n ? bad(ctx, "k / ox is null") : ECSIMD_HIP_OK;
  if (generator ? (x || y) : (!x || !y)) return bad(ctx, "a base point array is missing (or BASE_GENERATOR came with one)");
  if (!affine && (!oy || !oz)) return bad(ctx, "a Jacobian result needs ox, oy and oz");
  if (n == 0) return ECSIMD_HIP_OK;
  if (capturing(ctx)) return bad(ctx, "scalar_mult_host copies and synchronises: not inside a stream capture");
  (void)hipSetDevice(ctx->device);
  const size_t chunk = n < HOST_CHUNK ? n : HOST_CHUNK, chunks = (n + chunk - 1) / chunk;
  if (chunks > 1 && !ctx->helper) { int rc = ecsimd_hip_init(ctx->device, &ctx->helper); if (rc != ECSIMD_HIP_OK) return bad(ctx, "scalar_mult_host: the helper context could not be created"); }
  host_side S[2];
  for (int i = 0; i < (chunks > 1 ? 2 : 1); ++i) {
    ecsimd_hip_ctx* c = i == 0 ? ctx : ctx->helper;
    c->ref_square = ctx->ref_square;
    int rc = host_stage(c, chunk, 6, &S[i]);
    if (rc != ECSIMD_HIP_OK) { if (c != ctx) snprintf(ctx->err, sizeof ctx->err, "%s", c->err); return rc; }
  }
  auto report = [&](ecsimd_hip_ctx* c, int rc) { if (c != ctx) snprintf(ctx->err, sizeof ctx->err, "%s", c->err); return rc; };
  auto launch = [&](size_t ci) -> int {
    host_side& s = S[ci & 1];
    const size_t first = ci * chunk, m = (n - first) < chunk ? (n - first) : chunk;
    int rc = ecsimd_hip_memcpy_h2d(s.c, s.k, k + 4 * first, m * 32);
    if (rc == ECSIMD_HIP_OK && !generator) rc = ecsimd_hip_memcpy_h2d(s.c, s.x, x + 4 * first, m * 32);
    if (rc == ECSIMD_HIP_OK && !generator) rc = ecsimd_hip_memcpy_h2d(s.c, s.y, y + 4 * first, m * 32);
    if (rc == ECSIMD_HIP_OK) rc = ecsimd_hip_scalar_mult(s.c, curve, s.k, generator ? nullptr : s.x, generator ? nullptr : s.y, s.o[0], oy ? s.o[1] : nullptr, affine ? nullptr : s.o[2], m, flags);
    return report(s.c, rc);
  };
  auto drain = [&](size_t ci) -> int {
    host_side& s = S[ci & 1];
    const size_t first = ci * chunk, m = (n - first) < chunk ? (n - first) : chunk;
    int rc = ecsimd_hip_memcpy_d2h(s.c, ox + 4 * first, s.o[0], m * 32);               // (waits for this side's kernels, then copies)
    if (rc == ECSIMD_HIP_OK && oy) rc = ecsimd_hip_memcpy_d2h(s.c, oy + 4 * first, s.o[1], m * 32);
    if (rc == ECSIMD_HIP_OK && !affine) rc = ecsimd_hip_memcpy_d2h(s.c, oz + 4 * first, s.o[2], m * 32);
    return report(s.c, rc);
  };
  for (size_t ci = 0; ci <= chunks; ++ci) {
    if (ci < chunks) { int rc = launch(ci); if (rc != ECSIMD_HIP_OK) { if (ci > 0) (void)ecsimd_hip_sync(S[(ci - 1) & 1].c); return rc; } }
    if (ci > 0) { int rc = drain(ci - 1); if (rc != ECSIMD_HIP_OK) return rc; }
  }
  return ECSIMD_HIP_OK;
}
int ecsimd_hip_scalar_mult_1s(ecsimd_hip_ctx* ctx, int curve, const uint64_t k1[4], const uint64_t* x, const uint64_t* y, uint64_t* ox, uint64_t* oy, uint64_t* oz, size_t n, int flags) {
  REQUIRE_CTX(); REQUIRE_PTR(x); REQUIRE_PTR(y); REQUIRE_PTR(ox); REQUIRE_OUT_Y(oy); if (!k1) return bad(ctx, "k1 is null");
  if (!(flags & ECSIMD_HIP_OUT_AFFINE)) REQUIRE_PTR(oz);
  if (curve < ECSIMD_HIP_FIRST_REGISTERED_CURVE) REQUIRE_CURVE();
  uint32_t* kdev = ctx->sink + 1024 - 8;    // 32-byte aligned slot at the end of the scratch page
  ENTER_ANY_SIZE();
  store_words(ctx->stream, words8_of(k1), kdev);
  return variable_base_mult(ctx, curve, reinterpret_cast<const uint64_t*>(kdev), 0, x, y, ox, oy, oz, n, flags); }
int ecsimd_hip_scalar_mult_base(ecsimd_hip_ctx* ctx, int curve, const uint64_t* k, uint64_t* ox, uint64_t* oy, uint64_t* oz, size_t n, int flags) {
  REQUIRE_CTX(); REQUIRE_PTR(k); REQUIRE_PTR(ox); REQUIRE_OUT_Y(oy);
  flags &= ~ECSIMD_HIP_BASE_GENERATOR;                            // (implied here)
  if (!(flags & ECSIMD_HIP_OUT_AFFINE)) REQUIRE_PTR(oz);
  if (curve >= ECSIMD_HIP_FIRST_REGISTERED_CURVE) {
    int rc = gc_small_base(ctx, curve, k, ox, oy, n, flags);       // small batches, affine output, no algorithm asked for: the constant-time comb, the ladder's bits kept
    if (rc != GC_NOT_TAKEN) return rc;
    return run_gladder(ctx, curve, k, 4, nullptr, nullptr, ox, oy, oz, n, flags & ~ECSIMD_HIP_BASE_MGRY);
  }
  REQUIRE_CURVE();
  if (flags & (ECSIMD_HIP_ALG_WINDOWED | ECSIMD_HIP_ALG_WINDOWED_SIGNED | ECSIMD_HIP_ALG_WINDOWED_BIG)) {
    const bool big = (flags & ECSIMD_HIP_ALG_WINDOWED_BIG) != 0;         // signed 20-bit windows, table in device memory
    const bool six = (flags & ECSIMD_HIP_ALG_WINDOWED_SIGNED) != 0;      // signed 7-bit windows, table in LDS
    // windows over a precomputed table, then one simultaneous inversion: affine output only
    // (the Jacobian representative differs from the reference ladder's -- SURVEY.md 8(a) level A).
    if (!(flags & ECSIMD_HIP_OUT_AFFINE)) return bad(ctx, "ALG_WINDOWED needs OUT_AFFINE");
    const bool ct = (flags & ECSIMD_HIP_ALG_CONSTANT_TIME) != 0;
    if (ct && (big || six)) return bad(ctx, "ALG_CONSTANT_TIME modifies ALG_WINDOWED only (its own 5-bit comb in LDS), not ALG_WINDOWED_SIGNED / ALG_WINDOWED_BIG");
    NO_COMPAT("ALG_WINDOWED");
    ENTER();
    jacobian j;
    int rc = ensure_window_table(ctx, curve, big ? launch::BIG_WINDOW_BITS : six ? SIGNED_WBITS : ct ? CT_WBITS : 4);    // ALG_CONSTANT_TIME: its own 5-bit comb
    if (rc == ECSIMD_HIP_OK) rc = ensure_jacobian(ctx, n, &j);
    if (rc != ECSIMD_HIP_OK) return rc;
    hipStream_t s = ctx->stream;
    if (ct) secret_base_product(ctx, curve, k, j, ox, oy, n);            // (no wipe: the product is the call's result, in the caller's arrays)
    else {
      if (big) launch::base_windowed_big(s, curve, k, ctx->window16_table[curve], j.x, j.y, j.z, n);
      else if (six) launch::base_windowed_signed(s, curve, k, ctx->window6_table[curve], j.x, j.y, j.z, n, false);
      else launch::base_windowed(s, curve, k, ctx->window_table[curve], j.x, j.y, j.z, n, false);
      launch::to_affine_batched(s, curve, j.x, j.y, j.z, ox, oy, n, true);
    }
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? ECSIMD_HIP_OK : fail(ctx, e, "scalar_mult_base (windowed) launch");
  }
  if (flags & ECSIMD_HIP_ALG_CONSTANT_TIME) return bad(ctx, "ALG_CONSTANT_TIME modifies ALG_WINDOWED (the ladder is constant-time as it is)");
  // Small batches, affine output, no algorithm asked for: a launch of the ladder costs its 254 iterations however few lanes it has (1.3 ms), the
  // constant-time comb 51 additions (0.2 ms) -- and every reference test and benchmark multiplies G (benchs/curve_group.cpp:23-35).  The comb is as
  // safe for secret scalars as the ladder; its affine result is the true k*G, which is the ladder's everywhere but at the ladder's three degenerate
  // scalars, and there the lanes take the ladder's own (meaningless, but the reference's) coordinates from a 288-byte record: the same bits out.
  if ((flags & ECSIMD_HIP_OUT_AFFINE) && n <= SMALL_BASE_MAX && !(flags & (ECSIMD_HIP_REF_SQUARE_COMPAT | ECSIMD_HIP_LADDER_RADIX32)) && !ctx->ref_square &&
      !capturing_needs_build(ctx, curve)) {
    ENTER_ANY_SIZE();                                                       // (n <= SMALL_BASE_MAX)
    jacobian j;
    int rc = ensure_window_table(ctx, curve, CT_WBITS);
    const bool x_is_exact = (oy == nullptr && curve == ECSIMD_HIP_P256);    // the P-256 x-only ladder returns the true x for every k already
    if (rc == ECSIMD_HIP_OK && !x_is_exact) rc = ensure_base_special(ctx, curve);
    if (rc == ECSIMD_HIP_OK) rc = ensure_jacobian(ctx, n, &j);
    if (rc != ECSIMD_HIP_OK) return rc;
    secret_base_product(ctx, curve, k, j, ox, oy, n);                       // (no wipe, as in the ALG_CONSTANT_TIME branch above)
    if (!x_is_exact) launch::patch_special(ctx->stream, k, ctx->base_special[curve], ox, oy, n);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? ECSIMD_HIP_OK : fail(ctx, e, "scalar_mult_base (small batch) launch");
  }
  return run_ladder(ctx, curve, k, 4, nullptr, nullptr, ox, oy, oz, n, flags); }
int ecsimd_hip_affine_add(ecsimd_hip_ctx* ctx, int curve, const uint64_t* ax, const uint64_t* ay, const uint64_t* bx, const uint64_t* by,
                          uint64_t* rx, uint64_t* ry, uint8_t* finite, size_t n) {
  REQUIRE_CTX(); if (curve < ECSIMD_HIP_FIRST_REGISTERED_CURVE) REQUIRE_CURVE(); REQUIRE_PTR(ax); REQUIRE_PTR(ay); REQUIRE_PTR(bx); REQUIRE_PTR(by); REQUIRE_PTR(rx);
  if (ry && !aligned16(ry)) return bad(ctx, "ry is not 16-byte aligned");
  if (any_alias({rx}, {ax, ay, bx, by})) return bad(ctx, "rx must not alias an input (it is the inversion scratch)");
  GENERIC_CURVE(launch::gc_affine_add_batched(s, GC, ax, ay, bx, by, rx, ry, finite, n));
  RUN(launch::affine_add_batched(s, curve, ax, ay, bx, by, rx, ry, finite, n)); }

// u1[i]*G + u2[i]*Q[i]: windowed fixed-base product + windowed variable-base product + one batched affine
// addition, in chunks of VARWIN_CHUNK elements.  Every Q[i] is validated first (x, y < p, on the curve; the point at
// infinity (0, 0) fails): an invalid public key yields the point at infinity and finite[i] = 0 -- without the check
// the window tables of such a lane would hold multiples on some other curve and the result would look like a point.
// u1*G comes from the 20-bit window table in device memory (436 MB per curve, built on first use) once that table
// exists or the batch is large enough to pay for building it; smaller batches take the signed 7-bit table in LDS.
namespace {
// per chunk: the Jacobian u1 G, the affine u1 G and u2 Q, the window loop's per-lane tables
struct dsm_layout { size_t chunk; jacobian j; uint64_t *gx, *gy, *px, *py, *tables; size_t bytes; };
dsm_layout dsm_plan(void* base, size_t n) {
  dsm_layout L; L.chunk = chunk_of(n, VARWIN_CHUNK);
  carve c = carve_from(base);
  L.j = carve_jacobian(c, L.chunk); L.gx = carve_limbs(c, L.chunk); L.gy = carve_limbs(c, L.chunk); L.px = carve_limbs(c, L.chunk); L.py = carve_limbs(c, L.chunk);
  L.tables = static_cast<uint64_t*>(carve_bytes(c, launch::varwin_scratch_bytes(L.chunk)));
  L.bytes = c.bytes;
  return L;
}
// The caller has gone through ENTER; `reserve_behind` bytes behind the layout are the caller's and stay untouched.
int double_scalar_mult_impl(ecsimd_hip_ctx* ctx, int curve, const uint64_t* u1, const uint64_t* u2, const uint64_t* qx, const uint64_t* qy,
                            uint64_t* rx, uint64_t* ry, uint8_t* finite, size_t n, size_t reserve_behind, const uint8_t* known_valid = nullptr) {
  // known_valid (ecdsa_recover): the caller built every Q[i] from the curve equation and says which lanes count -- no second validation pass
  int rc = public_base_product(ctx, curve, n);
  if (rc == ECSIMD_HIP_OK) rc = ensure_workspace(ctx, dsm_plan(nullptr, n).bytes + reserve_behind);
  if (rc == ECSIMD_HIP_OK && !known_valid) rc = ensure_valid(ctx, flag_bytes(n));
  if (rc != ECSIMD_HIP_OK) return rc;
  const dsm_layout L = dsm_plan(ctx->workspace, n);
  hipStream_t s = ctx->stream;
  if (!known_valid) launch::on_curve(s, curve, qx, qy, ctx->valid, n);
  FOR_CHUNKS(first, m, n, L.chunk) {
    (void)public_base_product(ctx, curve, n, u1 + 4 * first, &L.j, m);                                          // u1*G (the table is there)
    launch::to_affine_batched(s, curve, L.j.x, L.j.y, L.j.z, L.gx, L.gy, m, true);
    launch::varwin_scalar_mult(s, curve, u2 + 4 * first, 4, qx + 4 * first, qy + 4 * first, ECSIMD_HIP_BASE_CLASSICAL, L.tables, L.px, L.py, m);   // u2*Q
    launch::affine_add_batched(s, curve, L.gx, L.gy, L.px, L.py, rx + 4 * first, ry ? ry + 4 * first : nullptr, finite ? finite + first : nullptr, m);
  }
  launch::clear_invalid(s, known_valid ? known_valid : ctx->valid, rx, ry, finite, n);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? ECSIMD_HIP_OK : fail(ctx, e, "double_scalar_mult launch");
}
}  // namespace

// ---- u1 G + u2 Q, ECDSA verification and signing on a curve registered at run time: with the group order (n >= 2^255) u1 G from the generator's comb
// (k_gcomb.hip) and u2 Q from the lane's own window table (k_gvarwin.hip: verification's scalars are public); a ladder pass (gc_safe_mult) stands in for u2 Q where n is not a
// checked prime order, and for u1 G where the comb's table does not exist yet and a stream capture forbids building it -- ECDSA asks n >= 2^255 -- the
// scalars kept clear of its degenerate values (three, as n >= 2^255 is asked at registration: k_gc_ladder_safe_scalars); one shared inversion per product, a batched affine addition.
namespace {
constexpr size_t GC_CHUNK = (size_t)1 << 22;
constexpr size_t GC_BIG_COMB_WORTH_IT = (size_t)1 << 20;          // u1 G + u2 Q on a registered curve: batches from here on build the 20-bit comb (0.3 s, 436 MB) on first use
struct gc_layout { size_t chunk; uint64_t *adj1, *adj2, *j[3], *gx, *gy, *px, *py, *win; uint8_t *neg1, *neg2; size_t bytes; };
// win: u2 Q goes through the window loop (k_gvarwin.hip), whose per-lane tables follow the nine arrays
gc_layout gc_plan(uint64_t* base, size_t n, bool win = false) {
  gc_layout L; L.chunk = chunk_of(n, GC_CHUNK);
  carve c = carve_from(base);
  L.adj1 = carve_limbs(c, L.chunk); L.adj2 = carve_limbs(c, L.chunk); for (int i = 0; i < 3; ++i) L.j[i] = carve_limbs(c, L.chunk);
  L.gx = carve_limbs(c, L.chunk); L.gy = carve_limbs(c, L.chunk); L.px = carve_limbs(c, L.chunk); L.py = carve_limbs(c, L.chunk);
  L.win = win ? static_cast<uint64_t*>(carve_bytes(c, launch::gc_varwin_scratch_bytes(L.chunk))) : nullptr;
  L.neg1 = carve_flags(c, L.chunk); L.neg2 = carve_flags(c, L.chunk);
  L.bytes = c.bytes;
  return L;
}
// The comb of a registered curve (k_gcomb.hip): 64 windows x 8 odd multiples (2d + 1) 16^w G, then k* G and the record {k*, 0} (k_affine.inc comb_special's
// layout).  Needs the order (the recoding works modulo n) with n >= 2^255 (k mod n by one subtraction).  Every entry comes from the reference's ladder on this
// curve -- whose degenerate scalars the entries' multipliers must not be (checked; k* by way of n - k* if it is one) -- through the shared inversion.
bool gc_comb_possible(const curve_record& rec) { return rec.has_order && (rec.n.l[3] >> 63) != 0 && !rec.order_wrong; }
bool gc_window_possible(const curve_record& rec) { return gc_comb_possible(rec) && rec.prime_order; }    // a variable base: every point has order n (curve_record)
// bits = 4: that table (summed from the top); bits = 7 / 5 / 20: the signed comb's 37 windows x 64 / the constant-time comb's 52 windows x 16 / the device-memory
// comb's 13 windows x 2^19 (436 MB; 1.3 GB of temporary memory and 6.8 M ladder passes, ~0.3 s, at its build) odd multiples (2d + 1) 2^(bits w) G (summed from
// the bottom; the top window's digit is at most 15 / 1 / 65 535: its other entries are never read and hold G).
int ensure_gc_comb(ecsimd_hip_ctx* ctx, int curve, const curve_record& rec, const uint32_t** out, int bits = 4) {
  auto slot = [bits](ecsimd_hip_ctx::gcomb_entry& t) -> uint32_t*& { return bits == 4 ? t.table : bits == 7 ? t.table7 : bits == 20 ? t.table20 : t.table5; };
  for (auto& t : ctx->gcomb) if (t.curve == curve && slot(t)) { *out = slot(t); return ECSIMD_HIP_OK; }
  if (!gc_comb_possible(rec)) return bad(ctx, "the windowed algorithms on a registered curve need its group order n, n >= 2^255 (and n G = O where n is a prime in p's Hasse interval)");
  if (capturing(ctx)) return bad(ctx, "a window table would have to be built during stream capture: run this call once before capturing");
  static_assert(launch::GCOMB_WINDOWS == 64 && launch::GCOMB_ENTRIES == 8 && launch::GCOMB7_WINDOWS == 37 && launch::GCOMB7_ENTRIES == 64 && launch::GCOMB5_WINDOWS == 52 &&
                launch::GCOMB5_ENTRIES == 16 && launch::GCOMB20_WINDOWS == 13 && launch::GCOMB20_ENTRIES == 1 << 19, "plan_comb: ceil(256 / bits) windows x 2^(bits - 1) entries");
  comb_plan P;
  int rc = plan_comb(ctx, rec.n, bits, P);
  if (rc != ECSIMD_HIP_OK) return rc;
  try { ctx->gcomb.reserve(ctx->gcomb.size() + 1); } catch (...) { return bad(ctx, "window table: out of host memory"); }
  const size_t table_entries = P.table_entries, entries = P.entries;
  (void)hipSetDevice(ctx->device);
  uint64_t* kd = nullptr;
  uint32_t* table = nullptr;
  hipError_t e = hipMalloc(&kd, 6 * entries * 32 + 64);
  if (e == hipSuccess) e = hipMalloc(&table, (entries + 1) * 64);
  uint64_t* tx = kd + entries * 4; uint64_t* ty = tx + entries * 4;
  uint64_t* jx = ty + entries * 4; uint64_t* jy = jx + entries * 4; uint64_t* jz = jy + entries * 4;
  uint8_t* flag = reinterpret_cast<uint8_t*>(jz + entries * 4);
  if (e == hipSuccess) e = hipMemcpyAsync(kd, P.k.data(), entries * 32, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipMemsetAsync(flag, 1, 16, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);          // P.k must outlive the copy
  if (e == hipSuccess) {
    launch::gc_scalar_mult(ctx->stream, rec.G, kd, 4, nullptr, nullptr, jx, jy, jz, entries, 0);
    launch::gc_to_affine_batched(ctx->stream, rec.G, jx, jy, jz, tx, ty, entries);
    if (P.negate_special) launch::gc_negate_where(ctx->stream, rec.G, flag, ty + table_entries * 4, 1);
    launch::gc_pack_table(ctx->stream, rec.G, tx, ty, table, (int)entries);
    e = hipMemcpyAsync(table + entries * 16, P.kstar, 64, hipMemcpyHostToDevice, ctx->stream);
  }
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e == hipSuccess) e = hipGetLastError();
  (void)hipFree(kd);
  if (e != hipSuccess) { (void)hipFree(table); return fail(ctx, e, "window table build (registered curve)"); }
  bool placed = false;
  for (auto& t : ctx->gcomb) if (t.curve == curve) { slot(t) = table; placed = true; }
  if (!placed) { ctx->gcomb.push_back({curve, nullptr, nullptr, nullptr, nullptr, nullptr}); slot(ctx->gcomb.back()) = table; }
  *out = table;
  return ECSIMD_HIP_OK;
}
// The small-batch route's record for a registered curve (ensure_base_special for the built-in ones): n - 1, 2^256 - n - 1, 2^256 - n and what the reference's
// ladder returns for them on G, affine -- computed by the very launches run_gladder(OUT_AFFINE) makes.
int ensure_gc_base_special(ecsimd_hip_ctx* ctx, int curve, const curve_record& rec, const uint64_t** out) {
  for (auto& t : ctx->gcomb) if (t.curve == curve && t.special) { *out = t.special; return ECSIMD_HIP_OK; }
  if (capturing(ctx)) return bad(ctx, "a record would have to be built during stream capture: run this call once before capturing");
  u256 s3[3]; ladder_degenerate_points(rec.n, s3);
  uint64_t host[12];
  for (int j = 0; j < 3; ++j) for (int l = 0; l < 4; ++l) host[4 * j + l] = s3[j].l[l];
  uint64_t* r = nullptr; uint64_t* tmp = nullptr;
  hipError_t e = hipMalloc(&r, 9 * 32);
  if (e == hipSuccess) e = hipMalloc(&tmp, 9 * 32);
  if (e == hipSuccess) e = hipMemcpyAsync(r, host, 3 * 32, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e == hipSuccess) {
    launch::gc_scalar_mult(ctx->stream, rec.G, r, 4, nullptr, nullptr, tmp, tmp + 12, tmp + 24, 3, 0);
    launch::gc_to_affine_batched(ctx->stream, rec.G, tmp, tmp + 12, tmp + 24, r + 12, r + 24, 3);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  }
  (void)hipFree(tmp);
  if (e != hipSuccess) { (void)hipFree(r); return fail(ctx, e, "base_special build (registered curve)"); }
  for (auto& t : ctx->gcomb) if (t.curve == curve) { t.special = r; *out = r; return ECSIMD_HIP_OK; }
  (void)hipFree(r);
  return bad(ctx, "base_special: the curve's table is missing");
}
launch::words8 order_words(const curve_record& rec) { return words8_of(rec.n.l); }
}  // namespace
namespace {
// scalar_mult_base(registered curve, ALG_WINDOWED [| ALG_CONSTANT_TIME] | OUT_AFFINE): the comb, then the shared inversion -- the true k G for every k
// (k mod n = 0: (0, 0)), which is the ladder's affine result everywhere but at the ladder's degenerate scalars.
int run_gcomb(ecsimd_hip_ctx* ctx, int curve, const uint64_t* k, uint64_t* ox, uint64_t* oy, size_t n, int flags) {
  if (!(flags & ECSIMD_HIP_OUT_AFFINE)) return bad(ctx, "ALG_WINDOWED needs OUT_AFFINE");
  if (ctx->ref_square || (flags & (ECSIMD_HIP_REF_SQUARE_COMPAT | ECSIMD_HIP_LADDER_RADIX32))) return bad(ctx, "ALG_WINDOWED is not the reference's algorithm: no ECSIMD_HIP_REF_SQUARE_COMPAT / LADDER_RADIX32 form");
  curve_record rec; if (!lookup_curve_record(curve, &rec)) return bad(ctx, "unknown curve id");
  if (n == 0) return gc_comb_possible(rec) ? ECSIMD_HIP_OK : bad(ctx, "the windowed algorithms on a registered curve need its group order n, n >= 2^255 (and n G = O where n is a prime in p's Hasse interval)");
  ENTER();
  const uint32_t* table = nullptr; jacobian j;
  const bool seven = (flags & ECSIMD_HIP_ALG_WINDOWED_SIGNED) != 0;     // signed 7-bit windows in 148 KiB of LDS: 36 additions instead of 63 (public scalars)
  const bool big = (flags & ECSIMD_HIP_ALG_WINDOWED_BIG) != 0;          // 20-bit windows over 436 MB in device memory: 12 additions (public scalars)
  const bool five = !seven && !big && (flags & ECSIMD_HIP_ALG_CONSTANT_TIME) != 0;   // the constant-time comb: 5-bit windows, 51 additions, every entry of a window read
  int rc = ensure_gc_comb(ctx, curve, rec, &table, seven ? 7 : big ? 20 : five ? 5 : 4);
  if (rc == ECSIMD_HIP_OK) rc = ensure_jacobian(ctx, n, &j);
  if (rc != ECSIMD_HIP_OK) return rc;
  if (seven || five || big) launch::gc_base_windowed_s(ctx->stream, rec.G, order_words(rec), seven ? 7 : big ? 20 : 5, k, table, j.x, j.y, j.z, n);
  else launch::gc_base_windowed(ctx->stream, rec.G, order_words(rec), k, table, j.x, j.y, j.z, n, false);
  launch::gc_to_affine_batched(ctx->stream, rec.G, j.x, j.y, j.z, ox, oy, n);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? ECSIMD_HIP_OK : fail(ctx, e, "scalar_mult_base (registered curve, windowed) launch");
}
// scalar_mult(registered curve, ALG_WINDOWED [| ALG_CONSTANT_TIME] | OUT_AFFINE) on a variable base: per-lane tables of the eight odd multiples of P over one Z, the
// window loop on the isomorphic curve (k_gvarwin.hip), then the shared inversion -- the true k P for every k (k = 0 mod n: (0, 0)).  In chunks of 2^22 lanes
// (640 B of scratch per lane).  `reserve` bytes at the start of the workspace stay untouched (gc_double_scalar_mult).
int run_gvarwin(ecsimd_hip_ctx* ctx, int curve, const uint64_t* k, int k_stride, const uint64_t* x, const uint64_t* y, uint64_t* ox, uint64_t* oy, size_t n, int flags, size_t reserve) {
  if (!(flags & ECSIMD_HIP_OUT_AFFINE)) return bad(ctx, "ALG_WINDOWED needs OUT_AFFINE");
  NO_COMPAT("ALG_WINDOWED");
  if (flags & ECSIMD_HIP_LADDER_RADIX32) return bad(ctx, "LADDER_RADIX32 selects a ladder loop: not with ALG_WINDOWED");
  curve_record rec; if (!lookup_curve_record(curve, &rec)) return bad(ctx, "unknown curve id");
  if (!gc_comb_possible(rec)) return bad(ctx, "the windowed algorithms on a registered curve need its group order n, n >= 2^255 (and n G = O where n is a prime in p's Hasse interval)");
  if (!gc_window_possible(rec)) return bad(ctx, "ALG_WINDOWED on a variable base needs a group of prime order: n is not a prime in p's Hasse interval (the ladder has no such condition)");
  ENTER_ANY_SIZE();
  const size_t chunk = chunk_of(n, VARWIN_CHUNK);
  int rc = ensure_workspace(ctx, reserve + launch::gc_varwin_scratch_bytes(chunk));
  if (rc != ECSIMD_HIP_OK) return rc;
  uint64_t* scratch = ctx->workspace + reserve / 8;
  FOR_CHUNKS(first, m, n, chunk)
    launch::gc_varwin_scalar_mult(ctx->stream, rec.G, order_words(rec), k + (size_t)k_stride * first, k_stride, x + 4 * first, y + 4 * first, flags & (ECSIMD_HIP_BASE_MGRY | ECSIMD_HIP_ALG_CONSTANT_TIME),
                                  scratch, ox + 4 * first, oy ? oy + 4 * first : nullptr, m);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? ECSIMD_HIP_OK : fail(ctx, e, "scalar_mult (registered curve, windowed) launch");
}
// scalar_mult_base(registered curve, OUT_AFFINE, no ALG_* / ladder flag) on up to 2^16 lanes: as for the built-in curves (ecsimd_hip_scalar_mult_base below) a
// ladder launch costs its 254 iterations however few lanes it has; the constant-time comb costs 63 additions.  Its affine result is the true k G -- the ladder's
// everywhere but at the ladder's three degenerate scalars, and there the lanes take the ladder's own coordinates from the record: the same bits out.
int gc_small_base(ecsimd_hip_ctx* ctx, int curve, const uint64_t* k, uint64_t* ox, uint64_t* oy, size_t n, int flags) {
  constexpr int other = ECSIMD_HIP_REF_SQUARE_COMPAT | ECSIMD_HIP_LADDER_RADIX32 | ECSIMD_HIP_ALG_WINDOWED | ECSIMD_HIP_ALG_WINDOWED_SIGNED | ECSIMD_HIP_ALG_WINDOWED_BIG |
                        ECSIMD_HIP_ALG_NO_ENDOMORPHISM | ECSIMD_HIP_ALG_CONSTANT_TIME;
  if (!(flags & ECSIMD_HIP_OUT_AFFINE) || (flags & other) || ctx->ref_square || n == 0 || n > SMALL_BASE_MAX) return GC_NOT_TAKEN;
  curve_record rec; if (!lookup_curve_record(curve, &rec) || !gc_comb_possible(rec)) return GC_NOT_TAKEN;
  (void)hipSetDevice(ctx->device);
  const uint32_t* table = nullptr; const uint64_t* special = nullptr;
  int rc = ensure_gc_comb(ctx, curve, rec, &table);
  if (rc == ECSIMD_HIP_OK) rc = ensure_gc_base_special(ctx, curve, rec, &special);
  if (rc != ECSIMD_HIP_OK) { ctx->err[0] = 0; return GC_NOT_TAKEN; }                     // (a capture in progress and nothing built yet, a curve whose table cannot be built: the ladder)
  if (capturing(ctx) && ctx->workspace_bytes < jacobian_bytes(n)) return GC_NOT_TAKEN;
  jacobian j; rc = ensure_jacobian(ctx, n, &j);
  if (rc != ECSIMD_HIP_OK) return rc;
  hipStream_t s = ctx->stream;
  launch::gc_base_windowed(s, rec.G, order_words(rec), k, table, j.x, j.y, j.z, n, true);
  launch::gc_to_affine_batched(s, rec.G, j.x, j.y, j.z, ox, oy, n);
  launch::patch_special(s, k, special, ox, oy, n);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? ECSIMD_HIP_OK : fail(ctx, e, "scalar_mult_base (registered curve, small batch) launch");
}
int gc_require_ecdsa(ecsimd_hip_ctx* ctx, int curve, curve_record* rec) {
  if (!lookup_curve_record(curve, rec)) return bad(ctx, "unknown curve id");
  if (!rec->has_order) return bad(ctx, "this curve was registered without its group order n");
  if (rec->order_wrong) return bad(ctx, "ECDSA on a registered curve needs its group order n, n >= 2^255: this n is a prime in p's Hasse interval and n G != O");
  if (!rec->ecdsa_ok) return bad(ctx, "ECDSA on a registered curve needs an order n >= 2^255 (the ladder's further degenerate scalars below it are not worked around), p < 2n, and n - u a good ladder scalar for the three degenerate u");
  if (wants_compat(ctx)) return refuse_compat(ctx, nullptr);
  return ECSIMD_HIP_OK;
}
// one product k P (P = G when x == nullptr) -> affine classical (ox, oy), correct for EVERY k < n; oy may be null (x only: the negation does not touch x)
void gc_safe_mult(hipStream_t s, const curve_record& rec, const gc_layout& L, uint64_t* adj, uint8_t* neg, const uint64_t* k, const uint64_t* x, const uint64_t* y, uint64_t* ox, uint64_t* oy, size_t m) {
  launch::gc_ladder_safe_scalars(s, rec.N, k, adj, neg, m);
  launch::gc_scalar_mult(s, rec.G, adj, 4, x, y, L.j[0], L.j[1], L.j[2], m, 0);
  launch::gc_to_affine_batched(s, rec.G, L.j[0], L.j[1], L.j[2], ox, oy, m);
  if (oy) launch::gc_negate_where(s, rec.G, neg, oy, m);
}
int gc_double_scalar_mult(ecsimd_hip_ctx* ctx, int curve_of, const curve_record& rec, const uint64_t* u1, const uint64_t* u2, const uint64_t* qx, const uint64_t* qy,
                          uint64_t* rx, uint64_t* ry, uint8_t* finite, size_t n, size_t reserve_behind, const uint8_t* known_valid = nullptr) {
  const bool win = gc_window_possible(rec);                         // u2 Q from the lane's own window table where the curve has a prime order n >= 2^255, else a ladder pass
  gc_layout L = gc_plan(nullptr, n, win);
  int rc = ensure_workspace(ctx, L.bytes + reserve_behind);
  if (rc == ECSIMD_HIP_OK && !known_valid) rc = ensure_valid(ctx, flag_bytes(n));
  if (rc != ECSIMD_HIP_OK) return rc;
  const uint32_t* comb = nullptr;                                  // u1 G from the generator's table where the curve has one (n >= 2^255), else a ladder pass
  const uint32_t* comb7 = nullptr;                                  // ... preferably the signed 7-bit comb (u1 is public: 36 additions instead of 63)
  const uint32_t* comb20 = nullptr;                                 // ... or the 20-bit comb in device memory (12 additions) once it exists or the batch pays for its 436 MB
  if (gc_comb_possible(rec)) {
    bool have20 = false;
    for (auto& t : ctx->gcomb) if (t.curve == curve_of && t.table20) have20 = true;
    if (have20 || (n >= GC_BIG_COMB_WORTH_IT && !capturing(ctx))) { rc = ensure_gc_comb(ctx, curve_of, rec, &comb20, 20); if (rc != ECSIMD_HIP_OK) comb20 = nullptr; }
    rc = comb20 ? ECSIMD_HIP_OK : ensure_gc_comb(ctx, curve_of, rec, &comb7, 7);
    if (rc != ECSIMD_HIP_OK) {
      if (!capturing(ctx)) return rc;
      comb7 = nullptr;
      rc = ensure_gc_comb(ctx, curve_of, rec, &comb); if (rc != ECSIMD_HIP_OK) comb = nullptr;      // (no table yet and a capture in progress: the other table, else the ladder)
    }
  }
  L = gc_plan(ctx->workspace, n, win);
  hipStream_t s = ctx->stream;
  if (!known_valid) launch::gc_on_curve(s, rec.G, qx, qy, ctx->valid, n);      // (ecdsa_recover built every Q[i] from the curve equation: known_valid says which lanes count)
  FOR_CHUNKS(first, m, n, L.chunk) {
    if (comb20 || comb7 || comb) {
      if (comb20) launch::gc_base_windowed_s(s, rec.G, order_words(rec), 20, u1 + 4 * first, comb20, L.j[0], L.j[1], L.j[2], m);
      else if (comb7) launch::gc_base_windowed_s(s, rec.G, order_words(rec), 7, u1 + 4 * first, comb7, L.j[0], L.j[1], L.j[2], m);
      else launch::gc_base_windowed(s, rec.G, order_words(rec), u1 + 4 * first, comb, L.j[0], L.j[1], L.j[2], m, false);
      launch::gc_to_affine_batched(s, rec.G, L.j[0], L.j[1], L.j[2], L.gx, L.gy, m);
    } else gc_safe_mult(s, rec, L, L.adj1, L.neg1, u1 + 4 * first, nullptr, nullptr, L.gx, L.gy, m);                       // u1 G
    if (win) launch::gc_varwin_scalar_mult(s, rec.G, order_words(rec), u2 + 4 * first, 4, qx + 4 * first, qy + 4 * first, 0, L.win, L.px, L.py, m);   // u2 Q (public scalars)
    else gc_safe_mult(s, rec, L, L.adj2, L.neg2, u2 + 4 * first, qx + 4 * first, qy + 4 * first, L.px, L.py, m);
    launch::gc_affine_add_batched(s, rec.G, L.gx, L.gy, L.px, L.py, rx + 4 * first, ry ? ry + 4 * first : nullptr, finite ? finite + first : nullptr, m);
  }
  launch::clear_invalid(s, known_valid ? known_valid : ctx->valid, rx, ry, finite, n);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? ECSIMD_HIP_OK : fail(ctx, e, "double_scalar_mult (registered curve) launch");
}
// ECDSA's acceptance test on top of a double product: behind that product's own `front` bytes of the workspace, the sums' x coordinates and finite flags; behind
// those, `extra` bytes that stay untouched for the caller (ecdsa_verify's u1, u2 and range flags).
struct verify_layout { uint64_t* rx; uint8_t* fin; size_t behind; };
verify_layout verify_plan(void* base, size_t front, size_t n) {
  verify_layout V; carve c = carve_from(base);
  (void)carve_bytes(c, front); V.rx = carve_limbs(c, n); V.fin = carve_flags(c, n); V.behind = c.bytes - front;
  return V;
}
// ecdsa_verify's own arrays behind verify_plan's: u1 = e / s, u2 = r / s and the range flags
struct verify_scalars { uint64_t *u1, *u2; uint8_t* in_range; size_t extra; };
verify_scalars verify_scalars_plan(void* base, size_t front, size_t n) {
  verify_scalars S; carve c = carve_from(base);
  (void)carve_bytes(c, front); S.u1 = carve_limbs(c, n); S.u2 = carve_limbs(c, n); S.in_range = carve_flags(c, n); S.extra = c.bytes - front;
  return S;
}
int gc_ecdsa_verify_rx(ecsimd_hip_ctx* ctx, int curve_of, const curve_record& rec, const uint64_t* u1, const uint64_t* u2, const uint64_t* qx, const uint64_t* qy, const uint64_t* r, uint8_t* ok, size_t n, size_t extra) {
  const size_t front = gc_plan(nullptr, n, gc_window_possible(rec)).bytes, behind = verify_plan(nullptr, front, n).behind;
  int rc = ensure_workspace(ctx, front + behind + extra);
  if (rc != ECSIMD_HIP_OK) return rc;
  const verify_layout V = verify_plan(ctx->workspace, front, n);
  rc = gc_double_scalar_mult(ctx, curve_of, rec, u1, u2, qx, qy, V.rx, nullptr, V.fin, n, behind + extra);
  if (rc != ECSIMD_HIP_OK) return rc;
  launch::gc_x_mod_n_equals(ctx->stream, rec.N, V.rx, V.fin, r, ok, n);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? ECSIMD_HIP_OK : fail(ctx, e, "ecdsa_verify_rx (registered curve) launch");
}
}  // namespace

int ecsimd_hip_on_curve(ecsimd_hip_ctx* ctx, int curve, const uint64_t* x, const uint64_t* y, uint8_t* ok, size_t n) {
  REQUIRE_CTX(); REQUIRE_PTR(x); REQUIRE_PTR(y); if (!ok && n) return bad(ctx, "ok is null");
  GENERIC_CURVE(launch::gc_on_curve(s, GC, x, y, ok, n));
  REQUIRE_CURVE(); RUN(launch::on_curve(s, curve, x, y, ok, n)); }

int ecsimd_hip_double_scalar_mult(ecsimd_hip_ctx* ctx, int curve, const uint64_t* u1, const uint64_t* u2, const uint64_t* qx, const uint64_t* qy,
                                  uint64_t* rx, uint64_t* ry, uint8_t* finite, size_t n) {
  REQUIRE_CTX(); REQUIRE_PTR(u1); REQUIRE_PTR(u2); REQUIRE_PTR(qx); REQUIRE_PTR(qy); REQUIRE_PTR(rx);
  if (ry && !aligned16(ry)) return bad(ctx, "ry is not 16-byte aligned");
  if (curve >= ECSIMD_HIP_FIRST_REGISTERED_CURVE) {
    curve_record rec; int rc = gc_require_ecdsa(ctx, curve, &rec); if (rc != ECSIMD_HIP_OK) return rc;
    ENTER_ANY_SIZE();
    return gc_double_scalar_mult(ctx, curve, rec, u1, u2, qx, qy, rx, ry, finite, n, 0);
  }
  REQUIRE_CURVE();
  if (wants_compat(ctx)) return refuse_compat(ctx, "double_scalar_mult");
  ENTER_ANY_SIZE();
  return double_scalar_mult_impl(ctx, curve, u1, u2, qx, qy, rx, ry, finite, n, 0); }

// ECDSA's acceptance test on top of double_scalar_mult: ok[i] = Q[i] is a valid public key && u1*G + u2*Q is finite && its x mod n == r[i].
namespace {
int ecdsa_verify_rx_impl(ecsimd_hip_ctx* ctx, int curve, const uint64_t* u1, const uint64_t* u2, const uint64_t* qx, const uint64_t* qy,
                         const uint64_t* r, uint8_t* ok, size_t n, size_t extra) {
  const size_t front = dsm_plan(nullptr, n).bytes, behind = verify_plan(nullptr, front, n).behind;
  // sizes the workspace (and builds the table) first, so that the pointers taken below stay valid
  int rc = public_base_product(ctx, curve, n);
  if (rc == ECSIMD_HIP_OK) rc = ensure_workspace(ctx, front + behind + extra);
  if (rc != ECSIMD_HIP_OK) return rc;
  const verify_layout V = verify_plan(ctx->workspace, front, n);
  rc = double_scalar_mult_impl(ctx, curve, u1, u2, qx, qy, V.rx, nullptr, V.fin, n, behind + extra);
  if (rc != ECSIMD_HIP_OK) return rc;
  launch::x_mod_n_equals(ctx->stream, curve, V.rx, V.fin, r, ok, n);       // fin is 0 for the lanes whose Q failed validation
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? ECSIMD_HIP_OK : fail(ctx, e, "ecdsa_verify_rx launch");
}
}  // namespace

int ecsimd_hip_ecdsa_verify_rx(ecsimd_hip_ctx* ctx, int curve, const uint64_t* u1, const uint64_t* u2, const uint64_t* qx, const uint64_t* qy,
                               const uint64_t* r, uint8_t* ok, size_t n) {
  REQUIRE_CTX(); REQUIRE_PTR(u1); REQUIRE_PTR(u2); REQUIRE_PTR(qx); REQUIRE_PTR(qy); REQUIRE_PTR(r);
  if (!ok && n) return bad(ctx, "ok is null");
  if (curve >= ECSIMD_HIP_FIRST_REGISTERED_CURVE) {
    curve_record rec; int rc = gc_require_ecdsa(ctx, curve, &rec); if (rc != ECSIMD_HIP_OK) return rc;
    ENTER_ANY_SIZE();
    return gc_ecdsa_verify_rx(ctx, curve, rec, u1, u2, qx, qy, r, ok, n, 0);
  }
  REQUIRE_CURVE();
  if (wants_compat(ctx)) return refuse_compat(ctx, "ecdsa_verify_rx");
  ENTER_ANY_SIZE();
  return ecdsa_verify_rx_impl(ctx, curve, u1, u2, qx, qy, r, ok, n, 0); }

// The whole verification (SEC 1 v2 4.1.4, FIPS 186-5 6.4.2): range checks and u1 = e / s, u2 = r / s modulo the group order on the device
// (k_gfield.hip k_ecdsa_scalars: one shared inversion per up to 128 signatures), then the acceptance test above.
int ecsimd_hip_ecdsa_verify(ecsimd_hip_ctx* ctx, int curve, const uint64_t* e, const uint64_t* r, const uint64_t* s_, const uint64_t* qx, const uint64_t* qy,
                            uint8_t* ok, size_t n) {
  REQUIRE_CTX(); REQUIRE_PTR(e); REQUIRE_PTR(r); REQUIRE_PTR(s_); REQUIRE_PTR(qx); REQUIRE_PTR(qy);
  if (!ok && n) return bad(ctx, "ok is null");
  if (curve >= ECSIMD_HIP_FIRST_REGISTERED_CURVE) {
    // the same verification on a registered curve: u1, u2 modulo ITS order (the record's field of n), then two ladders, an affine addition, x mod n = r
    curve_record rec; int rc = gc_require_ecdsa(ctx, curve, &rec); if (rc != ECSIMD_HIP_OK) return rc;
    ENTER();
    const size_t front = gc_plan(nullptr, n, gc_window_possible(rec)).bytes, inner = front + verify_plan(nullptr, front, n).behind;
    rc = ensure_workspace(ctx, inner + verify_scalars_plan(nullptr, inner, n).extra);
    if (rc != ECSIMD_HIP_OK) return rc;
    const verify_scalars S = verify_scalars_plan(ctx->workspace, inner, n);
    launch::ecdsa_scalars(ctx->stream, rec.N, e, r, s_, S.u1, S.u2, S.in_range, n);
    rc = gc_ecdsa_verify_rx(ctx, curve, rec, S.u1, S.u2, qx, qy, r, ok, n, S.extra);
    if (rc != ECSIMD_HIP_OK) return rc;
    launch::mask_op(ctx->stream, ECSIMD_HIP_MASK_AND, ok, S.in_range, ok, n);
    hipError_t err = hipGetLastError();
    return err == hipSuccess ? ECSIMD_HIP_OK : fail(ctx, err, "ecdsa_verify (registered curve) launch");
  }
  REQUIRE_CURVE();
  if (wants_compat(ctx)) return refuse_compat(ctx, "ecdsa_verify");
  ENTER();
  group_order O; int rc = builtin_order(ctx, curve, &O); if (rc != ECSIMD_HIP_OK) return rc;
  const size_t front = dsm_plan(nullptr, n).bytes, inner = front + verify_plan(nullptr, front, n).behind;
  rc = public_base_product(ctx, curve, n);
  if (rc == ECSIMD_HIP_OK) rc = ensure_workspace(ctx, inner + verify_scalars_plan(nullptr, inner, n).extra);
  if (rc != ECSIMD_HIP_OK) return rc;
  const verify_scalars S = verify_scalars_plan(ctx->workspace, inner, n);
  launch::ecdsa_scalars(ctx->stream, O.N, e, r, s_, S.u1, S.u2, S.in_range, n);
  rc = ecdsa_verify_rx_impl(ctx, curve, S.u1, S.u2, qx, qy, r, ok, n, S.extra);     // the workspace is already this large: nothing moves
  if (rc != ECSIMD_HIP_OK) return rc;
  launch::mask_op(ctx->stream, ECSIMD_HIP_MASK_AND, ok, S.in_range, ok, n);      // u1 = u2 = 0 already fails (the sum is infinite); the flag says why
  hipError_t err = hipGetLastError();
  return err == hipSuccess ? ECSIMD_HIP_OK : fail(ctx, err, "ecdsa_verify launch"); }

// Signing: R = k G on the constant-time comb (the kernel behind ALG_WINDOWED | ALG_CONSTANT_TIME), then the scalar-field half.  v == nullptr (ecdsa_sign): x(R)
// only.  Otherwise (ecdsa_sign_recoverable) y(R) is kept through the simultaneous inversion and k_recover.hip's select-only kernel adds
// v = parity(y) | (x >= n ? 2 : 0) and the low-s rule; the affine y joins the Jacobian k G and x in the workspace and is zeroed with them.
namespace {
struct sign_layout { jacobian j; uint64_t *rx, *ry; size_t bytes; };     // the Jacobian k G, x(k G) and, for the recovery id, y(k G)
sign_layout sign_plan(void* base, size_t n, bool keep_y) {
  sign_layout L; carve c = carve_from(base);
  L.j = carve_jacobian(c, n); L.rx = carve_limbs(c, n); L.ry = keep_y ? carve_limbs(c, n) : nullptr; L.bytes = c.bytes;
  return L;
}
int ecdsa_sign_builtin(ecsimd_hip_ctx* ctx, int curve, const uint64_t* e, const uint64_t* d, const uint64_t* k, uint64_t* r, uint64_t* s_, uint8_t* v, uint8_t* ok, size_t n, bool low_s) {
  ENTER();
  group_order O; int rc = builtin_order(ctx, curve, &O); if (rc != ECSIMD_HIP_OK) return rc;
  rc = ensure_window_table(ctx, curve, CT_WBITS);
  if (rc == ECSIMD_HIP_OK) rc = ensure_workspace(ctx, sign_plan(nullptr, n, v != nullptr).bytes);
  if (rc != ECSIMD_HIP_OK) return rc;
  const sign_layout L = sign_plan(ctx->workspace, n, v != nullptr);
  secret_base_product(ctx, curve, k, L.j, L.rx, L.ry, n);
  launch::ecdsa_sign_scalars(ctx->stream, O.N, e, d, k, L.rx, r, s_, ok, n);
  if (v) launch::sign_recovery_id(ctx->stream, O.words, L.rx, L.ry, s_, ok, v, n, low_s);
  const hipError_t err = wipe_workspace(ctx, L.bytes, hipGetLastError());
  return err == hipSuccess ? ECSIMD_HIP_OK : fail(ctx, err, v ? "ecdsa_sign_recoverable launch" : "ecdsa_sign launch");
}
// On a registered curve: k G from the constant-time comb of its generator (k_gcomb.hip: 5-bit windows, every entry of a window read) where the curve has one; else,
// and where no table exists yet and a capture in progress forbids building it, through the reference's ladder, constant-time as it is (tests/test_constant_time_isa.py
// holds both to the ISA); the select-only shared inversion; then the scalar-field kernel with the record's order.  One launch: at most 2^22 signatures.
int ecdsa_sign_registered(ecsimd_hip_ctx* ctx, int curve, const curve_record& rec, const uint64_t* e, const uint64_t* d, const uint64_t* k, uint64_t* r, uint64_t* s_, uint8_t* v, uint8_t* ok,
                          size_t n, bool low_s) {
  ENTER();
  gc_layout L = gc_plan(nullptr, n);
  if (L.chunk != n) return bad(ctx, v ? "ecdsa_sign_recoverable on a registered curve: at most 2^22 signatures per call" : "ecdsa_sign on a registered curve: at most 2^22 signatures per call");
  int rc = ensure_workspace(ctx, L.bytes);
  if (rc != ECSIMD_HIP_OK) return rc;
  const uint32_t* comb = nullptr;
  if (gc_comb_possible(rec)) { rc = ensure_gc_comb(ctx, curve, rec, &comb, 5); if (rc != ECSIMD_HIP_OK) { if (!capturing(ctx)) return rc; comb = nullptr; } }
  L = gc_plan(ctx->workspace, n);
  uint64_t* ry = v ? L.gy : nullptr;
  if (comb) {
    launch::gc_base_windowed_s(ctx->stream, rec.G, order_words(rec), 5, k, comb, L.j[0], L.j[1], L.j[2], n);
    launch::gc_to_affine_batched(ctx->stream, rec.G, L.j[0], L.j[1], L.j[2], L.gx, ry, n);
  } else gc_safe_mult(ctx->stream, rec, L, L.adj1, L.neg1, k, nullptr, nullptr, L.gx, ry, n);          // (the negation of a degenerate nonce's product does not touch x)
  launch::ecdsa_sign_scalars(ctx->stream, rec.N, e, d, k, L.gx, r, s_, ok, n);
  if (v) launch::sign_recovery_id(ctx->stream, order_words(rec), L.gx, L.gy, s_, ok, v, n, low_s);
  const hipError_t err = wipe_workspace(ctx, L.bytes, hipGetLastError());                              // the nonce's adjusted copy, the Jacobian k G and the affine point
  return err == hipSuccess ? ECSIMD_HIP_OK : fail(ctx, err, v ? "ecdsa_sign_recoverable (registered curve) launch" : "ecdsa_sign (registered curve) launch");
}
}  // namespace

int ecsimd_hip_ecdsa_sign(ecsimd_hip_ctx* ctx, int curve, const uint64_t* e, const uint64_t* d, const uint64_t* k, uint64_t* r, uint64_t* s_, uint8_t* ok, size_t n) {
  REQUIRE_CTX(); REQUIRE_PTR(e); REQUIRE_PTR(d); REQUIRE_PTR(k); REQUIRE_PTR(r); REQUIRE_PTR(s_);
  if (!ok && n) return bad(ctx, "ok is null");
  curve_record rec;
  if (curve >= ECSIMD_HIP_FIRST_REGISTERED_CURVE) { int rc = gc_require_ecdsa(ctx, curve, &rec); if (rc != ECSIMD_HIP_OK) return rc; }
  else { REQUIRE_CURVE(); if (wants_compat(ctx)) return refuse_compat(ctx, "ecdsa_sign"); }
  if (any_alias({r, s_}, {e, d, k})) return bad(ctx, "r and s must not alias an input or each other");
  return curve >= ECSIMD_HIP_FIRST_REGISTERED_CURVE ? ecdsa_sign_registered(ctx, curve, rec, e, d, k, r, s_, nullptr, ok, n, false) : ecdsa_sign_builtin(ctx, curve, e, d, k, r, s_, nullptr, ok, n, false); }

// Public-key recovery (SEC 1 v2 4.1.6): R = (r + (v >> 1) n, the root of that parity) from k_recover.hip's lift, u1 = -e / r and u2 = s / r from its
// scalar-field kernel, then u1 G + u2 R through double_scalar_mult's window loops, whose validation of R is skipped: R was just built from the curve
// equation and the validity byte already says which lanes count.  ok = that byte && the sum is finite; (0, 0) elsewhere.  All data is public.
namespace {
// behind the double product's `front` bytes, per element of a chunk: u1, u2, the lifted R and `more` further arrays, then the validity byte and `more_flags` further byte arrays
struct recover_layout { uint64_t *u1, *u2, *px, *py, *more[2]; uint8_t *valid, *more_flags; size_t extra; };
recover_layout recover_plan(void* base, size_t front, size_t m, int more = 0, bool more_flags = false) {
  recover_layout L; carve c = carve_from(base);
  (void)carve_bytes(c, front); L.u1 = carve_limbs(c, m); L.u2 = carve_limbs(c, m); L.px = carve_limbs(c, m); L.py = carve_limbs(c, m);
  for (int i = 0; i < 2; ++i) L.more[i] = i < more ? carve_limbs(c, m) : nullptr;
  L.valid = carve_flags(c, m); L.more_flags = more_flags ? carve_flags(c, m) : nullptr;
  L.extra = c.bytes - front;
  return L;
}
}  // namespace
int ecsimd_hip_ecdsa_recover(ecsimd_hip_ctx* ctx, int curve, const uint64_t* e, const uint64_t* r, const uint64_t* s_, const uint8_t* v,
                             uint64_t* qx, uint64_t* qy, uint8_t* ok, size_t n) {
  REQUIRE_CTX(); REQUIRE_PTR(e); REQUIRE_PTR(r); REQUIRE_PTR(s_); REQUIRE_PTR(qx);
  if ((!v || !ok) && n) return bad(ctx, "v or ok is null");
  if (qy && !aligned16(qy)) return bad(ctx, "qy is not 16-byte aligned");
  if (curve >= ECSIMD_HIP_FIRST_REGISTERED_CURVE) {
    curve_record rec; int rc = gc_require_ecdsa(ctx, curve, &rec); if (rc != ECSIMD_HIP_OK) return rc;
    ENTER();
    const size_t front = gc_plan(nullptr, n, gc_window_possible(rec)).bytes;
    rc = ensure_workspace(ctx, front + recover_plan(nullptr, front, n).extra);
    if (rc != ECSIMD_HIP_OK) return rc;
    const recover_layout L = recover_plan(ctx->workspace, front, n);
    launch::gc_recover_lift(ctx->stream, rec.G, order_words(rec), r, v, L.px, L.py, L.valid, n);
    launch::ecdsa_recover_scalars(ctx->stream, rec.N, e, r, s_, L.u1, L.u2, L.valid, n);
    return gc_double_scalar_mult(ctx, curve, rec, L.u1, L.u2, L.px, L.py, qx, qy, ok, n, L.extra, L.valid);
  }
  REQUIRE_CURVE();
  if (wants_compat(ctx)) return refuse_compat(ctx, "ecdsa_recover");
  ENTER();
  group_order O; int rc = builtin_order(ctx, curve, &O); if (rc != ECSIMD_HIP_OK) return rc;
  const size_t front = dsm_plan(nullptr, n).bytes;
  // sizes the workspace (and builds the table) first, so that the pointers taken below stay valid
  rc = public_base_product(ctx, curve, n);
  if (rc == ECSIMD_HIP_OK) rc = ensure_workspace(ctx, front + recover_plan(nullptr, front, n).extra);
  if (rc != ECSIMD_HIP_OK) return rc;
  const recover_layout L = recover_plan(ctx->workspace, front, n);
  launch::recover_lift(ctx->stream, curve, O.words, r, v, L.px, L.py, L.valid, n);
  launch::ecdsa_recover_scalars(ctx->stream, O.N, e, r, s_, L.u1, L.u2, L.valid, n);
  return double_scalar_mult_impl(ctx, curve, L.u1, L.u2, L.px, L.py, qx, qy, ok, n, L.extra, L.valid); }

int ecsimd_hip_ecdsa_sign_recoverable(ecsimd_hip_ctx* ctx, int curve, const uint64_t* e, const uint64_t* d, const uint64_t* k, uint64_t* r, uint64_t* s_, uint8_t* v, uint8_t* ok,
                                      size_t n, int flags) {
  REQUIRE_CTX(); REQUIRE_PTR(e); REQUIRE_PTR(d); REQUIRE_PTR(k); REQUIRE_PTR(r); REQUIRE_PTR(s_);
  if ((!v || !ok) && n) return bad(ctx, "v or ok is null");
  if (flags & ~ECSIMD_HIP_ECDSA_LOW_S) return bad(ctx, "ecdsa_sign_recoverable: unknown flag");
  if (n != 0 && any_alias({r, s_}, {e, d, k})) return bad(ctx, "r and s must not alias an input or each other");   // (an empty batch has no arrays to alias)
  const bool low_s = (flags & ECSIMD_HIP_ECDSA_LOW_S) != 0;
  if (curve >= ECSIMD_HIP_FIRST_REGISTERED_CURVE) {
    curve_record rec; int rc = gc_require_ecdsa(ctx, curve, &rec); if (rc != ECSIMD_HIP_OK) return rc;
    return ecdsa_sign_registered(ctx, curve, rec, e, d, k, r, s_, v, ok, n, low_s);
  }
  REQUIRE_CURVE();
  if (wants_compat(ctx)) return refuse_compat(ctx, "ecdsa_sign_recoverable");
  return ecdsa_sign_builtin(ctx, curve, e, d, k, r, s_, v, ok, n, low_s); }

// ---- SHA-256 and deterministic nonces (k_sha256.hip)
int ecsimd_hip_sha256(ecsimd_hip_ctx* ctx, const uint8_t* msg, size_t msg_bytes, size_t stride_bytes, uint64_t* e, size_t n) {
  REQUIRE_CTX(); REQUIRE_PTR(e);
  if (!msg && n && msg_bytes) return bad(ctx, "msg is null");
  if (stride_bytes < msg_bytes) return bad(ctx, "sha256: stride_bytes is smaller than msg_bytes");
  if (msg_bytes > ((size_t)1 << 40)) return bad(ctx, "sha256: message too long");
  RUN(launch::sha256(s, msg, msg_bytes, stride_bytes, e, n)); }

namespace {
// What the RFC 6979 kernels take from a curve: its order and C(n), the least C with (1 - n / 2^256)^C <= 2^-128 (double precision), which is the cap on
// the candidates a lane may try.  qlen = 256 only: n >= 2^255, so that a candidate is the 256 bits of one HMAC and C(n) <= 128.
struct nonce_plan { launch::words8 order; unsigned cap; };
unsigned rfc6979_candidates_needed(const u256& n) {
  u256 miss; const u256 zero = {{0, 0, 0, 0}};
  (void)u_sub(miss, zero, n);                                         // 2^256 - n
  double q = 0;
  for (int i = 3; i >= 0; --i) q = q * 18446744073709551616.0 + (double)miss.l[i];
  const double c = 128.0 / (256.0 - log2(q));
  return (unsigned)ceil(c);
}
int nonce_lookup(ecsimd_hip_ctx* ctx, int curve, nonce_plan* out) {
  u256 n;
  if (curve >= ECSIMD_HIP_FIRST_REGISTERED_CURVE) {
    curve_record rec; if (!lookup_curve_record(curve, &rec)) return bad(ctx, "unknown curve id");
    if (!rec.has_order) return bad(ctx, "RFC 6979 nonces need a curve registered with its group order n and the ECDSA capability");
    if (!gc_comb_possible(rec)) return bad(ctx, "RFC 6979 nonces are supported where qlen = 256: this curve's order is below 2^255");
    if (!rec.ecdsa_ok) return bad(ctx, "RFC 6979 nonces need a curve registered with its group order n and the ECDSA capability");
    n = rec.n;
  } else {
    REQUIRE_CURVE();
    n = order_of(curve);
  }
  out->order = words8_of(n.l);
  out->cap = rfc6979_candidates_needed(n);
  return ECSIMD_HIP_OK;
}
// per element behind `front` bytes of a chunk: the nonce (32 B), K as two midstates and V (96 B), the retry byte, a recovery id nobody asked for
struct nonce_layout { uint64_t* k; void* state; uint8_t* retry; uint8_t* v; size_t bytes; };
nonce_layout nonce_plan_ws(uint64_t* base, size_t front, size_t m) {
  nonce_layout L; carve c = carve_from(base);
  (void)carve_bytes(c, front); L.k = carve_limbs(c, m); L.state = carve_bytes(c, 96 * m); L.retry = carve_flags(c, m); L.v = carve_flags(c, m);
  L.bytes = c.bytes - front;
  return L;
}
}  // namespace

int ecsimd_hip_rfc6979_nonce(ecsimd_hip_ctx* ctx, int curve, const uint64_t* e, const uint64_t* d, uint64_t* k, uint8_t* ok, size_t n) {
  REQUIRE_CTX(); REQUIRE_PTR(e); REQUIRE_PTR(d); REQUIRE_PTR(k);
  if (!ok && n) return bad(ctx, "ok is null");
  nonce_plan P; int rc = nonce_lookup(ctx, curve, &P); if (rc != ECSIMD_HIP_OK) return rc;
  if (n != 0 && any_alias({k}, {e, d})) return bad(ctx, "k must not alias an input");
  ENTER_ANY_SIZE();
  const size_t chunk = chunk_of(n, GC_CHUNK);
  rc = ensure_workspace(ctx, nonce_plan_ws(nullptr, 0, chunk).bytes);
  if (rc != ECSIMD_HIP_OK) return rc;
  hipError_t err = hipSuccess;
  FOR_CHUNKS(first, m, n, chunk) {
    const nonce_layout L = nonce_plan_ws(ctx->workspace, 0, m);
    launch::rfc6979_nonce(ctx->stream, P.order, e + 4 * first, d + 4 * first, k + 4 * first, L.state, L.retry, ok + first, m, P.cap);
    err = wipe_workspace(ctx, L.bytes, hipGetLastError());       // K, V and the retry bytes: gone before the call returns (L.k is unused here)
    if (err != hipSuccess) break;
  }
  return err == hipSuccess ? ECSIMD_HIP_OK : fail(ctx, err, "rfc6979_nonce launch"); }

// Deterministic signing: the nonce kernels write k into the context workspace, behind what ecdsa_sign_recoverable uses of it; then that call as it is -- the
// constant-time comb, the simultaneous inversion, ecdsa_sign_scalars, sign_recovery_id -- so the output is the chain's, bit for bit.  At most 2^22 elements at a time.
int ecsimd_hip_ecdsa_sign_deterministic(ecsimd_hip_ctx* ctx, int curve, const uint64_t* e, const uint64_t* d, uint64_t* r, uint64_t* s_, uint8_t* v, uint8_t* ok, size_t n, int flags) {
  REQUIRE_CTX(); REQUIRE_PTR(e); REQUIRE_PTR(d); REQUIRE_PTR(r); REQUIRE_PTR(s_);
  if (!ok && n) return bad(ctx, "ok is null");
  if (flags & ~ECSIMD_HIP_ECDSA_LOW_S) return bad(ctx, "ecdsa_sign_deterministic: unknown flag");
  nonce_plan P; int rc = nonce_lookup(ctx, curve, &P); if (rc != ECSIMD_HIP_OK) return rc;
  if (wants_compat(ctx)) return refuse_compat(ctx, "ecdsa_sign_deterministic");
  if (n != 0 && any_alias({r, s_}, {e, d})) return bad(ctx, "r and s must not alias an input or each other");
  ENTER_ANY_SIZE();
  const size_t chunk = chunk_of(n, GC_CHUNK);
  const size_t front = curve >= ECSIMD_HIP_FIRST_REGISTERED_CURVE ? gc_plan(nullptr, chunk).bytes : sign_plan(nullptr, chunk, true).bytes;     // ecdsa_sign_recoverable's own use of the workspace
  // the first call per curve builds the comb's table and sizes the workspace: both before any pointer into the block is taken
  rc = ensure_workspace(ctx, front + nonce_plan_ws(nullptr, 0, chunk).bytes);
  if (rc != ECSIMD_HIP_OK) return rc;
  FOR_CHUNKS(first, m, n, chunk) {
    const nonce_layout L = nonce_plan_ws(ctx->workspace, front, m);
    launch::rfc6979_nonce(ctx->stream, P.order, e + 4 * first, d + 4 * first, L.k, L.state, L.retry, ok + first, m, P.cap);
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) return fail(ctx, err, "ecdsa_sign_deterministic launch");
    rc = ecsimd_hip_ecdsa_sign_recoverable(ctx, curve, e + 4 * first, d + 4 * first, L.k, r + 4 * first, s_ + 4 * first, v ? v + first : L.v, ok + first, m, flags);
    // K, V, the last candidate and the nonce (and the unwanted v) are zeroed whatever the signing step said
    err = hipMemsetAsync(L.k, 0, L.bytes, ctx->stream);
    if (rc != ECSIMD_HIP_OK) return rc;
    if (err != hipSuccess) return fail(ctx, err, "ecdsa_sign_deterministic: zeroing the workspace");
  }
  return ECSIMD_HIP_OK; }

// ---- Keccak-256, Ethereum addresses and address recovery (k_keccak.hip); public data throughout
int ecsimd_hip_keccak256(ecsimd_hip_ctx* ctx, const uint8_t* msg, size_t msg_bytes, size_t stride_bytes, const uint32_t* lens, uint64_t* e, size_t n) {
  REQUIRE_CTX(); REQUIRE_PTR(e);
  if (lens) msg_bytes = 0;                                                        // (ignored: every lane has its own length)
  if (!msg && n && (msg_bytes || (lens && stride_bytes))) return bad(ctx, "msg is null");
  if (lens && (reinterpret_cast<uintptr_t>(lens) & 3u)) return bad(ctx, "lens is not 4-byte aligned");
  if (stride_bytes < msg_bytes) return bad(ctx, "keccak256: stride_bytes is smaller than msg_bytes");
  if (msg_bytes > ((size_t)1 << 40)) return bad(ctx, "keccak256: message too long");
  RUN(launch::keccak256(s, msg, msg_bytes, stride_bytes, lens, e, n)); }

int ecsimd_hip_eth_address(ecsimd_hip_ctx* ctx, const uint64_t* qx, const uint64_t* qy, uint8_t* addr, size_t n) {
  REQUIRE_CTX(); REQUIRE_PTR(qx); REQUIRE_PTR(qy);
  if (!addr && n) return bad(ctx, "addr is null");
  if (reinterpret_cast<uintptr_t>(addr) & 3u) return bad(ctx, "addr is not 4-byte aligned");
  RUN(launch::eth_address(s, qx, qy, nullptr, addr, n)); }

// Per chunk: k_eth_recovery_id writes the recovery id the lift is to see (0xff where v, or the low-s rule, refuses the lane: the lift refuses every id above 3),
// then ecdsa_recover's chain as it is -- recover_lift, ecdsa_recover_scalars, double_scalar_mult_impl with the validity byte -- into the caller's qx / qy or
// into the workspace, then k_eth_address with the call's ok.  Behind the window loops' part of the workspace: u1, u2, R (four arrays), the key (two), two byte arrays.
int ecsimd_hip_eth_recover(ecsimd_hip_ctx* ctx, const uint64_t* e, const uint64_t* r, const uint64_t* s_, const uint8_t* v,
                           uint8_t* addr, uint64_t* qx, uint64_t* qy, uint8_t* ok, size_t n, int flags) {
  REQUIRE_CTX(); REQUIRE_PTR(e); REQUIRE_PTR(r); REQUIRE_PTR(s_);
  if ((!v || !ok || !addr) && n) return bad(ctx, "v, addr or ok is null");
  if (reinterpret_cast<uintptr_t>(addr) & 3u) return bad(ctx, "addr is not 4-byte aligned");
  if ((qx == nullptr) != (qy == nullptr)) return bad(ctx, "eth_recover: qx and qy are both given or both NULL");
  if (qx && (!aligned16(qx) || !aligned16(qy))) return bad(ctx, "qx or qy is not 16-byte aligned");
  if (flags & ~ECSIMD_HIP_ETH_REQUIRE_LOW_S) return bad(ctx, "eth_recover: unknown flag");
  if (wants_compat(ctx)) return refuse_compat(ctx, "eth_recover");
  ENTER();
  const int curve = ECSIMD_HIP_SECP256K1;
  group_order O; int rc = builtin_order(ctx, curve, &O); if (rc != ECSIMD_HIP_OK) return rc;
  launch::words8 half;
  for (int i = 0; i < 8; ++i) half.w[i] = (O.words.w[i] >> 1) | (i < 7 ? O.words.w[i + 1] << 31 : 0u);
  const size_t chunk = chunk_of(n, VARWIN_CHUNK), front = dsm_plan(nullptr, chunk).bytes;
  // sizes the workspace (and builds the table) first, so that the pointers taken below stay valid
  rc = public_base_product(ctx, curve, n);
  if (rc == ECSIMD_HIP_OK) rc = ensure_workspace(ctx, front + recover_plan(nullptr, front, chunk, 2, true).extra);
  if (rc != ECSIMD_HIP_OK) return rc;
  const recover_layout L = recover_plan(ctx->workspace, front, chunk, 2, true);      // more: the key where the caller does not want it; more_flags: the recovery id
  FOR_CHUNKS(first, m, n, chunk) {
    uint64_t* ox = qx ? qx + 4 * first : L.more[0]; uint64_t* oy = qy ? qy + 4 * first : L.more[1];
    launch::eth_recovery_id(ctx->stream, half, v + first, s_ + 4 * first, L.more_flags, m, (flags & ECSIMD_HIP_ETH_REQUIRE_LOW_S) != 0);
    launch::recover_lift(ctx->stream, curve, O.words, r + 4 * first, L.more_flags, L.px, L.py, L.valid, m);
    launch::ecdsa_recover_scalars(ctx->stream, O.N, e + 4 * first, r + 4 * first, s_ + 4 * first, L.u1, L.u2, L.valid, m);
    rc = double_scalar_mult_impl(ctx, curve, L.u1, L.u2, L.px, L.py, ox, oy, ok + first, m, L.extra, L.valid);
    if (rc != ECSIMD_HIP_OK) return rc;
    launch::eth_address(ctx->stream, ox, oy, ok + first, addr + 20 * first, m);
  }
  hipError_t err = hipGetLastError();
  return err == hipSuccess ? ECSIMD_HIP_OK : fail(ctx, err, "eth_recover launch"); }

// ---- Bitcoin: RIPEMD-160, HASH160, double SHA-256, public-key hashes (k_btc.hip); public data throughout, no workspace
namespace {
int btc_hash_args(ecsimd_hip_ctx* ctx, const char* what, const uint8_t* msg, size_t msg_bytes, size_t stride_bytes, const void* out, size_t n) {
  if (!out && n) return bad(ctx, "the output is null");
  if (!msg && n && msg_bytes) return bad(ctx, "msg is null");
  if (stride_bytes < msg_bytes || msg_bytes > ((size_t)1 << 40)) {
    snprintf(ctx->err, sizeof ctx->err, "bad argument: %s: %s", what, stride_bytes < msg_bytes ? "stride_bytes is smaller than msg_bytes" : "message too long");
    return ECSIMD_HIP_ERR_BAD_ARG;
  }
  return ECSIMD_HIP_OK;
}
}  // namespace

int ecsimd_hip_ripemd160(ecsimd_hip_ctx* ctx, const uint8_t* msg, size_t msg_bytes, size_t stride_bytes, uint8_t* out20, size_t n) {
  REQUIRE_CTX();
  int rc = btc_hash_args(ctx, "ripemd160", msg, msg_bytes, stride_bytes, out20, n); if (rc != ECSIMD_HIP_OK) return rc;
  if (reinterpret_cast<uintptr_t>(out20) & 3u) return bad(ctx, "out20 is not 4-byte aligned");
  RUN(launch::ripemd160(s, msg, msg_bytes, stride_bytes, out20, n)); }

int ecsimd_hip_hash160(ecsimd_hip_ctx* ctx, const uint8_t* msg, size_t msg_bytes, size_t stride_bytes, uint8_t* out20, size_t n) {
  REQUIRE_CTX();
  int rc = btc_hash_args(ctx, "hash160", msg, msg_bytes, stride_bytes, out20, n); if (rc != ECSIMD_HIP_OK) return rc;
  if (reinterpret_cast<uintptr_t>(out20) & 3u) return bad(ctx, "out20 is not 4-byte aligned");
  RUN(launch::hash160(s, msg, msg_bytes, stride_bytes, out20, n)); }

int ecsimd_hip_sha256d(ecsimd_hip_ctx* ctx, const uint8_t* msg, size_t msg_bytes, size_t stride_bytes, uint64_t* e, size_t n) {
  REQUIRE_CTX(); REQUIRE_PTR(e);
  int rc = btc_hash_args(ctx, "sha256d", msg, msg_bytes, stride_bytes, e, n); if (rc != ECSIMD_HIP_OK) return rc;
  RUN(launch::sha256d(s, msg, msg_bytes, stride_bytes, e, n)); }

int ecsimd_hip_btc_pubkey_hash(ecsimd_hip_ctx* ctx, const uint64_t* qx, const uint64_t* qy, uint8_t* out20, size_t n, int compressed) {
  REQUIRE_CTX(); REQUIRE_PTR(qx); REQUIRE_PTR(qy);
  if (!out20 && n) return bad(ctx, "out20 is null");
  if (reinterpret_cast<uintptr_t>(out20) & 3u) return bad(ctx, "out20 is not 4-byte aligned");
  RUN(launch::btc_pubkey_hash(s, qx, qy, out20, n, compressed != 0)); }

// ---- BIP-341 Taproot key tweaks on secp256k1 (k_btc.hip)
namespace {
// What xonly_tweak_chain and bip32_ckd_pub share, Q = P + t G between a front end and an accept kernel.  Per element of a chunk: the Jacobian sum (96 B), P, later
// the affine Q (64 B), t (32 B) and the validity byte.
struct tweak_layout { size_t chunk; jacobian j; uint64_t *x, *y, *t; uint8_t* valid; size_t bytes; };
tweak_layout tweak_plan(void* base, size_t n) {
  tweak_layout L; L.chunk = chunk_of(n, GC_CHUNK);
  carve c = carve_from(base);
  L.j = carve_jacobian(c, L.chunk); L.x = carve_limbs(c, L.chunk); L.y = carve_limbs(c, L.chunk); L.t = carve_limbs(c, L.chunk); L.valid = carve_flags(c, L.chunk);
  L.bytes = c.bytes;
  return L;
}
int tweak_prepare(ecsimd_hip_ctx* ctx, size_t n, tweak_layout* L) {
  int rc = public_base_product(ctx, ECSIMD_HIP_SECP256K1, n);
  if (rc == ECSIMD_HIP_OK) rc = ensure_workspace(ctx, tweak_plan(nullptr, n).bytes);
  if (rc == ECSIMD_HIP_OK) *L = tweak_plan(ctx->workspace, n);
  return rc;
}
// (x, y) + t G for m lanes of a batch of n: t G on the public comb, k_tweak_add, the inversion -- the spent point's place takes the affine sum, j.z stays for the accept kernel
void tweak_middle(ecsimd_hip_ctx* ctx, size_t n, const tweak_layout& L, size_t m) {
  (void)public_base_product(ctx, ECSIMD_HIP_SECP256K1, n, L.t, &L.j, m);
  launch::tweak_add(ctx->stream, L.j.x, L.j.y, L.j.z, L.x, L.y, m);
  launch::to_affine_batched(ctx->stream, ECSIMD_HIP_SECP256K1, L.j.x, L.j.y, L.j.z, L.x, L.y, m, true);
}
// Q = lift_x(px) + t G per chunk of 2^22: k_tweak_front (the lift, t given or hashed, the range check), t G on the public comb, k_tweak_add (complete: t = 0, the
// tangent, the opposite), ONE simultaneous inversion that keeps y, k_tweak_accept.
int xonly_tweak_chain(ecsimd_hip_ctx* ctx, const char* what, int mode, const uint64_t* px, const uint64_t* t_or_merkle, uint64_t* qx, uint8_t* parity, uint8_t* ok, size_t n) {
  if (wants_compat(ctx)) return refuse_compat(ctx, what);
  group_order O; int rc = builtin_order(ctx, ECSIMD_HIP_SECP256K1, &O); if (rc != ECSIMD_HIP_OK) return rc;
  ENTER_ANY_SIZE();
  tweak_layout L; rc = tweak_prepare(ctx, n, &L);
  if (rc != ECSIMD_HIP_OK) return rc;
  FOR_CHUNKS(first, m, n, L.chunk) {
    launch::tweak_front(ctx->stream, O.words, mode, px + 4 * first, t_or_merkle ? t_or_merkle + 4 * first : nullptr, L.x, L.y, L.t, L.valid, m);
    tweak_middle(ctx, n, L, m);
    launch::tweak_accept(ctx->stream, L.x, L.y, L.j.z, L.valid, qx + 4 * first, parity + first, ok + first, m);
  }
  hipError_t err = hipGetLastError();
  return err == hipSuccess ? ECSIMD_HIP_OK : fail(ctx, err, what);
}
}  // namespace

int ecsimd_hip_xonly_tweak_add(ecsimd_hip_ctx* ctx, const uint64_t* px, const uint64_t* t, uint64_t* qx, uint8_t* parity, uint8_t* ok, size_t n) {
  REQUIRE_CTX(); REQUIRE_PTR(px); REQUIRE_PTR(t); REQUIRE_PTR(qx);
  if ((!parity || !ok) && n) return bad(ctx, "parity or ok is null");
  if (n != 0 && any_alias({qx}, {px, t})) return bad(ctx, "qx must not alias an input");
  return xonly_tweak_chain(ctx, "xonly_tweak_add", launch::TWEAK_GIVEN, px, t, qx, parity, ok, n); }

int ecsimd_hip_taproot_tweak_pubkey(ecsimd_hip_ctx* ctx, const uint64_t* px, const uint64_t* merkle_root, uint64_t* qx, uint8_t* parity, uint8_t* ok, size_t n) {
  REQUIRE_CTX(); REQUIRE_PTR(px); REQUIRE_PTR(qx);
  if (merkle_root && !aligned16(merkle_root)) return bad(ctx, "merkle_root is not 16-byte aligned");
  if ((!parity || !ok) && n) return bad(ctx, "parity or ok is null");
  if (n != 0 && any_alias({qx}, {px, merkle_root})) return bad(ctx, "qx must not alias an input");
  return xonly_tweak_chain(ctx, "taproot_tweak_pubkey", merkle_root ? launch::TWEAK_MERKLE_ROOT : launch::TWEAK_KEY_PATH, px, merkle_root, qx, parity, ok, n); }

// The secret key of the output key: d G on the constant-time comb with both coordinates through the simultaneous inversion (secret_base_product),
// then k_taproot_seckey.  Per element of a chunk: the Jacobian product (96 B) and the affine d G (64 B) -- all zeroed behind the kernels (secret_base_product says why).
int ecsimd_hip_taproot_tweak_seckey(ecsimd_hip_ctx* ctx, const uint64_t* d, const uint64_t* merkle_root, uint64_t* d_out, uint64_t* px, uint8_t* ok, size_t n) {
  REQUIRE_CTX(); REQUIRE_PTR(d); REQUIRE_PTR(d_out);
  if ((merkle_root && !aligned16(merkle_root)) || (px && !aligned16(px))) return bad(ctx, "merkle_root or px is not 16-byte aligned");
  if (!ok && n) return bad(ctx, "ok is null");
  if (wants_compat(ctx)) return refuse_compat(ctx, "taproot_tweak_seckey");
  group_order O; int rc = builtin_order(ctx, ECSIMD_HIP_SECP256K1, &O); if (rc != ECSIMD_HIP_OK) return rc;
  if (n != 0 && any_alias({d_out, px}, {d, merkle_root})) return bad(ctx, "d_out and px must not alias an input or each other");
  ENTER_ANY_SIZE();
  const int curve = ECSIMD_HIP_SECP256K1;
  const size_t chunk = chunk_of(n, GC_CHUNK);
  rc = ensure_window_table(ctx, curve, CT_WBITS);
  if (rc == ECSIMD_HIP_OK) rc = ensure_workspace(ctx, sign_plan(nullptr, chunk, true).bytes);
  if (rc != ECSIMD_HIP_OK) return rc;
  const sign_layout L = sign_plan(ctx->workspace, chunk, true);              // the Jacobian d G and both affine coordinates
  hipError_t err = hipSuccess;
  FOR_CHUNKS(first, m, n, chunk) {
    secret_base_product(ctx, curve, d + 4 * first, L.j, L.rx, L.ry, m);
    launch::taproot_seckey(ctx->stream, O.N, d + 4 * first, merkle_root ? merkle_root + 4 * first : nullptr, L.rx, L.ry, d_out + 4 * first, px ? px + 4 * first : nullptr, ok + first, m);
    err = wipe_workspace(ctx, L.bytes, hipGetLastError());
    if (err != hipSuccess) break;
  }
  return err == hipSuccess ? ECSIMD_HIP_OK : fail(ctx, err, "taproot_tweak_seckey launch"); }

// ---- Bitcoin: one length per lane, Merkle roots, BIP-341 script paths (k_btc_tree.hip); public data throughout
namespace {
// btc_hash_args for a call with lens: msg_bytes does not count, the rows do
int btc_lens_args(ecsimd_hip_ctx* ctx, const char* what, const uint8_t* msg, size_t stride_bytes, const uint32_t* lens, const void* out, size_t n) {
  int rc = btc_hash_args(ctx, what, msg, 0, stride_bytes, out, n); if (rc != ECSIMD_HIP_OK) return rc;
  if (reinterpret_cast<uintptr_t>(lens) & 3u) return bad(ctx, "lens is not 4-byte aligned");
  if (!msg && n && stride_bytes) return bad(ctx, "msg is null");
  if (!stride_bytes && n > 1) return bad(ctx, "stride_bytes is 0 with lens: every lane would read the first row");
  return ECSIMD_HIP_OK;
}
}  // namespace

int ecsimd_hip_sha256_lens(ecsimd_hip_ctx* ctx, const uint8_t* msg, size_t msg_bytes, size_t stride_bytes, const uint32_t* lens, uint64_t* e, size_t n) {
  if (!lens) return ecsimd_hip_sha256(ctx, msg, msg_bytes, stride_bytes, e, n);
  REQUIRE_CTX(); REQUIRE_PTR(e);
  int rc = btc_lens_args(ctx, "sha256_lens", msg, stride_bytes, lens, e, n); if (rc != ECSIMD_HIP_OK) return rc;
  RUN(launch::sha256_lens(s, msg, stride_bytes, lens, e, n)); }

int ecsimd_hip_sha256d_lens(ecsimd_hip_ctx* ctx, const uint8_t* msg, size_t msg_bytes, size_t stride_bytes, const uint32_t* lens, uint64_t* e, size_t n) {
  if (!lens) return ecsimd_hip_sha256d(ctx, msg, msg_bytes, stride_bytes, e, n);
  REQUIRE_CTX(); REQUIRE_PTR(e);
  int rc = btc_lens_args(ctx, "sha256d_lens", msg, stride_bytes, lens, e, n); if (rc != ECSIMD_HIP_OK) return rc;
  RUN(launch::sha256d_lens(s, msg, stride_bytes, lens, e, n)); }

int ecsimd_hip_hash160_lens(ecsimd_hip_ctx* ctx, const uint8_t* msg, size_t msg_bytes, size_t stride_bytes, const uint32_t* lens, uint8_t* out20, size_t n) {
  if (!lens) return ecsimd_hip_hash160(ctx, msg, msg_bytes, stride_bytes, out20, n);
  REQUIRE_CTX();
  int rc = btc_lens_args(ctx, "hash160_lens", msg, stride_bytes, lens, out20, n); if (rc != ECSIMD_HIP_OK) return rc;
  if (reinterpret_cast<uintptr_t>(out20) & 3u) return bad(ctx, "out20 is not 4-byte aligned");
  RUN(launch::hash160_lens(s, msg, stride_bytes, lens, out20, n)); }

int ecsimd_hip_ripemd160_lens(ecsimd_hip_ctx* ctx, const uint8_t* msg, size_t msg_bytes, size_t stride_bytes, const uint32_t* lens, uint8_t* out20, size_t n) {
  if (!lens) return ecsimd_hip_ripemd160(ctx, msg, msg_bytes, stride_bytes, out20, n);
  REQUIRE_CTX();
  int rc = btc_lens_args(ctx, "ripemd160_lens", msg, stride_bytes, lens, out20, n); if (rc != ECSIMD_HIP_OK) return rc;
  if (reinterpret_cast<uintptr_t>(out20) & 3u) return bad(ctx, "out20 is not 4-byte aligned");
  RUN(launch::ripemd160_lens(s, msg, stride_bytes, lens, out20, n)); }

namespace {
// A chunk of whole trees: `trees` of them from tree `first`, `levels` launches; its node offsets are (levels + 1) rows of trees + 1 values from offsets[at] --
// row 0 the leaves' (into the caller's array), row l the nodes' behind l launches (from 0) -- and row `levels` has every tree at one node.
struct merkle_chunk { size_t first, trees, levels, at; };
// The chunks of a call and all their rows; p1 / p2 = the most nodes a chunk has behind its first / second launch.  Nothing may throw across the C ABI.
int merkle_plan(ecsimd_hip_ctx* ctx, const uint64_t* tree_offsets, size_t m, std::vector<merkle_chunk>& chunks, std::vector<uint64_t>& offsets, size_t* p1, size_t* p2) {
  *p1 = *p2 = 0;
  try {
    for (size_t t = 0; t < m;) {
      merkle_chunk c = {t, 0, 0, offsets.size()};
      uint64_t parents = 0, most = 0;
      for (; t < m; ++t, ++c.trees) {
        const uint64_t count = tree_offsets[t + 1] - tree_offsets[t];
        if (c.trees && parents + (count + 1) / 2 > GC_CHUNK) break;       // a tree larger than a chunk gets a chunk of its own
        parents += (count + 1) / 2;
        if (count > most) most = count;
      }
      for (uint64_t v = most; v > 1; v = (v + 1) / 2) ++c.levels;
      if (!c.levels) c.levels = 1;                                         // single leaves: one launch passes them through
      const size_t row = c.trees + 1;
      offsets.resize(c.at + (c.levels + 1) * row);
      uint64_t* o = &offsets[c.at];
      for (size_t q = 0; q < row; ++q) o[q] = tree_offsets[c.first + q];
      for (size_t l = 1; l <= c.levels; ++l) {
        const uint64_t* prev = o + (l - 1) * row; uint64_t* cur = o + l * row;
        cur[0] = 0;
        for (size_t q = 0; q < c.trees; ++q) cur[q + 1] = cur[q] + (prev[q + 1] - prev[q] + 1) / 2;
      }
      if (o[row + c.trees] > *p1) *p1 = o[row + c.trees];
      if (c.levels > 1 && o[2 * row + c.trees] > *p2) *p2 = o[2 * row + c.trees];
      chunks.push_back(c);
    }
  } catch (...) { return bad(ctx, "btc_merkle_root: out of host memory"); }
  return ECSIMD_HIP_OK;
}
// The pinned host block the rows are uploaded from: the copy is stream-ordered, so the block is the context's and the next upload waits for this one's event.
int merkle_stage(ecsimd_hip_ctx* ctx, const std::vector<uint64_t>& offsets, uint64_t* device) {
  const size_t bytes = offsets.size() * 8;
  hipError_t e = hipSuccess;
  if (!ctx->pinned_copied) e = hipEventCreateWithFlags(&ctx->pinned_copied, hipEventDisableTiming);
  else e = hipEventSynchronize(ctx->pinned_copied);
  if (e == hipSuccess && ctx->pinned_bytes < bytes) {
    if (ctx->pinned) (void)hipHostFree(ctx->pinned);
    ctx->pinned = nullptr; ctx->pinned_bytes = 0;
    e = hipHostMalloc(reinterpret_cast<void**>(&ctx->pinned), bytes, hipHostMallocDefault);
    if (e == hipSuccess) ctx->pinned_bytes = bytes;
  }
  if (e != hipSuccess) return fail(ctx, e, "btc_merkle_root: the pinned block of the node offsets");
  memcpy(ctx->pinned, offsets.data(), bytes);
  e = hipMemcpyAsync(device, ctx->pinned, bytes, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipEventRecord(ctx->pinned_copied, ctx->stream);
  return e == hipSuccess ? ECSIMD_HIP_OK : fail(ctx, e, "btc_merkle_root: uploading the node offsets");
}
}  // namespace

// Per chunk of whole trees: one launch per level.  Level 1 reads the caller's leaves, the levels between ping-pong in the workspace (odd levels in the first
// array, even ones in the second: every level is at most half the one two launches before it, rounded up per tree), the last one writes the caller's roots.
int ecsimd_hip_btc_merkle_root(ecsimd_hip_ctx* ctx, const uint64_t* leaves, const uint64_t* tree_offsets, size_t m, uint64_t* roots, uint8_t* mutated) {
  const size_t n = m;
  REQUIRE_CTX(); REQUIRE_PTR(leaves); REQUIRE_PTR(roots);
  if (!tree_offsets && n) return bad(ctx, "tree_offsets is null");
  for (size_t t = 0; t < m; ++t) {
    if (tree_offsets[t + 1] < tree_offsets[t]) return bad(ctx, "btc_merkle_root: tree_offsets decrease");
    if (tree_offsets[t + 1] == tree_offsets[t]) return bad(ctx, "btc_merkle_root: an empty tree");
  }
  if (n != 0 && any_alias({roots}, {leaves})) return bad(ctx, "roots must not alias leaves");
  ENTER_ANY_SIZE();
  if (capturing(ctx)) return bad(ctx, "btc_merkle_root stages its node offsets from host memory: not for a stream under capture");
  std::vector<merkle_chunk> chunks; std::vector<uint64_t> offsets; size_t p1, p2;
  int rc = merkle_plan(ctx, tree_offsets, m, chunks, offsets, &p1, &p2); if (rc != ECSIMD_HIP_OK) return rc;
  carve c = carve_from(nullptr);
  (void)carve_limbs(c, p1); (void)carve_limbs(c, p2); (void)carve_bytes(c, offsets.size() * 8);
  rc = ensure_workspace(ctx, c.bytes); if (rc != ECSIMD_HIP_OK) return rc;
  c = carve_from(ctx->workspace);
  uint64_t* level[2] = {carve_limbs(c, p1), carve_limbs(c, p2)};
  uint64_t* rows = static_cast<uint64_t*>(carve_bytes(c, offsets.size() * 8));
  rc = merkle_stage(ctx, offsets, rows); if (rc != ECSIMD_HIP_OK) return rc;
  hipError_t err = mutated ? hipMemsetAsync(mutated, 0, m, ctx->stream) : hipSuccess;
  if (err != hipSuccess) return fail(ctx, err, "btc_merkle_root: zeroing mutated");
  for (const merkle_chunk& k : chunks) {
    const size_t row = k.trees + 1;
    const uint64_t* in = leaves;
    for (size_t l = 1; l <= k.levels; ++l) {
      uint64_t* out = l == k.levels ? roots + 4 * k.first : level[(l - 1) & 1];
      launch::merkle_level(ctx->stream, in, rows + k.at + (l - 1) * row, rows + k.at + l * row, k.trees, out, mutated ? mutated + k.first : nullptr, offsets[k.at + l * row + k.trees]);
      in = out;
    }
  }
  err = hipGetLastError();
  return err == hipSuccess ? ECSIMD_HIP_OK : fail(ctx, err, "btc_merkle_root launch"); }

int ecsimd_hip_tapleaf_hash(ecsimd_hip_ctx* ctx, const uint8_t* script, size_t script_bytes, size_t stride_bytes, const uint32_t* lens, const uint8_t* leaf_version,
                            uint32_t leaf_version_all, uint64_t* e, size_t n) {
  REQUIRE_CTX(); REQUIRE_PTR(e);
  int rc = lens ? btc_lens_args(ctx, "tapleaf_hash", script, stride_bytes, lens, e, n) : btc_hash_args(ctx, "tapleaf_hash", script, script_bytes, stride_bytes, e, n);
  if (rc != ECSIMD_HIP_OK) return rc;
  if (!lens && script_bytes > 0xffffffffull) return bad(ctx, "tapleaf_hash: a script's length is below 2^32");
  if (!leaf_version && leaf_version_all > 0xffu) return bad(ctx, "tapleaf_hash: leaf_version_all is one byte");
  RUN(launch::tapleaf_hash(s, script, lens ? 0 : script_bytes, stride_bytes, lens, leaf_version, leaf_version_all, e, n)); }

int ecsimd_hip_taproot_merkle_path(ecsimd_hip_ctx* ctx, const uint64_t* leaf, const uint8_t* path, size_t path_stride_bytes, const uint8_t* depth, uint32_t depth_all,
                                   uint64_t* root, uint8_t* ok, size_t n) {
  REQUIRE_CTX(); REQUIRE_PTR(leaf); REQUIRE_PTR(root);
  if (!ok && n) return bad(ctx, "ok is null");
  if (!path && n && (depth || (depth_all != 0 && depth_all <= 128u))) return bad(ctx, "path is null");
  if (n != 0 && any_alias({root}, {leaf})) return bad(ctx, "root must not alias leaf");
  RUN(launch::taproot_merkle_path(s, leaf, path, path_stride_bytes, depth, depth_all, root, ok, n)); }

// ---- BIP-340 Schnorr signatures on secp256k1 (k_schnorr.hip)
namespace {
int schnorr_common(ecsimd_hip_ctx* ctx, const char* what, const uint8_t* msg, size_t msg_bytes, size_t stride_bytes, size_t n, group_order* O) {
  if (!msg && n && msg_bytes) return bad(ctx, "msg is null");
  if (stride_bytes < msg_bytes) return bad(ctx, "schnorr: stride_bytes is smaller than msg_bytes");
  if (msg_bytes > ((size_t)1 << 40)) return bad(ctx, "schnorr: message too long");
  if (wants_compat(ctx)) return refuse_compat(ctx, what);
  return builtin_order(ctx, ECSIMD_HIP_SECP256K1, O);
}
// The workspace of schnorr_verify_run for n signatures; verdicts_at: where the n verdict bytes of its ok == nullptr form begin (16-byte aligned), the last block.
size_t schnorr_verify_bytes(size_t n, bool verdicts_inside, size_t* verdicts_at = nullptr) {
  const size_t chunk = chunk_of(n, VARWIN_CHUNK), front = dsm_plan(nullptr, chunk).bytes;
  const size_t own = front + recover_plan(nullptr, front, chunk, 2, true).extra, aligned = (own + 15) / 16 * 16;
  if (verdicts_at) *verdicts_at = aligned;
  return verdicts_inside ? aligned + flag_bytes(n) : own;
}
// Verification of n >= 1 signatures, behind the argument checks and ENTER: k_schnorr_verify_front (the challenge, the lift, the range checks), then u1 G + u2 P
// through double_scalar_mult's window loops with the front end's validity byte (P was just built from the curve equation: no second validation pass), then
// k_schnorr_accept.  One chunk of 2^22 at a time, all in the workspace behind the window loops' own part: u1, u2, P, R (six arrays), the validity and the finite
// bytes.  ok == nullptr (schnorr_verify_batch's per-lane route): the verdict bytes go to the workspace, behind all of that, and *in_workspace is where.
int schnorr_verify_run(ecsimd_hip_ctx* ctx, const group_order& O, const uint64_t* px, const uint8_t* msg, size_t msg_bytes, size_t stride_bytes,
                       const uint64_t* r, const uint64_t* s_, uint8_t* ok, size_t n, uint8_t** in_workspace = nullptr) {
  const int curve = ECSIMD_HIP_SECP256K1;
  const size_t chunk = chunk_of(n, VARWIN_CHUNK), front = dsm_plan(nullptr, chunk).bytes;
  size_t verdicts_at = 0;
  // sizes the workspace (and builds the table) first, so that the pointers taken below stay valid
  int rc = public_base_product(ctx, curve, n);
  if (rc == ECSIMD_HIP_OK) rc = ensure_workspace(ctx, schnorr_verify_bytes(n, ok == nullptr, &verdicts_at));
  if (rc != ECSIMD_HIP_OK) return rc;
  if (!ok) ok = *in_workspace = reinterpret_cast<uint8_t*>(ctx->workspace) + verdicts_at;
  const recover_layout L = recover_plan(ctx->workspace, front, chunk, 2, true);      // px, py: the lifted P; more: R; more_flags: the sums' finite bytes
  FOR_CHUNKS(first, m, n, chunk) {
    launch::schnorr_verify_front(ctx->stream, O.words, px + 4 * first, r + 4 * first, s_ + 4 * first, msg ? msg + first * stride_bytes : nullptr, msg_bytes, stride_bytes, L.u1, L.u2, L.px, L.py, L.valid, m);
    rc = double_scalar_mult_impl(ctx, curve, L.u1, L.u2, L.px, L.py, L.more[0], L.more[1], L.more_flags, m, L.extra, L.valid);
    if (rc != ECSIMD_HIP_OK) return rc;
    launch::schnorr_accept(ctx->stream, L.more[0], L.more[1], L.more_flags, r + 4 * first, ok + first, m);
  }
  hipError_t err = hipGetLastError();
  return err == hipSuccess ? ECSIMD_HIP_OK : fail(ctx, err, "schnorr_verify launch"); }
}  // namespace

int ecsimd_hip_schnorr_verify(ecsimd_hip_ctx* ctx, const uint64_t* px, const uint8_t* msg, size_t msg_bytes, size_t stride_bytes,
                              const uint64_t* r, const uint64_t* s_, uint8_t* ok, size_t n) {
  REQUIRE_CTX(); REQUIRE_PTR(px); REQUIRE_PTR(r); REQUIRE_PTR(s_);
  if (!ok && n) return bad(ctx, "ok is null");
  group_order O;
  int rc = schnorr_common(ctx, "schnorr_verify", msg, msg_bytes, stride_bytes, n, &O); if (rc != ECSIMD_HIP_OK) return rc;
  ENTER_ANY_SIZE();
  return schnorr_verify_run(ctx, O, px, msg, msg_bytes, stride_bytes, r, s_, ok, n); }

// Signing: d G on the constant-time comb with both coordinates through the simultaneous inversion, k_schnorr_nonce, k0 G the same way, k_schnorr_finish.  Per
// element of a chunk: the Jacobian product (96 B, used twice), the affine d G and k0 G (64 B each), k0 (32 B) -- all zeroed behind the kernels (secret_base_product says why).
int ecsimd_hip_schnorr_sign(ecsimd_hip_ctx* ctx, const uint64_t* d, const uint8_t* msg, size_t msg_bytes, size_t stride_bytes,
                            const uint64_t* aux, uint64_t* px, uint64_t* r, uint64_t* s_, uint8_t* ok, size_t n) {
  REQUIRE_CTX(); REQUIRE_PTR(d); REQUIRE_PTR(r); REQUIRE_PTR(s_);
  if ((aux && !aligned16(aux)) || (px && !aligned16(px))) return bad(ctx, "aux or px is not 16-byte aligned");
  if (!ok && n) return bad(ctx, "ok is null");
  group_order O;
  int rc = schnorr_common(ctx, "schnorr_sign", msg, msg_bytes, stride_bytes, n, &O); if (rc != ECSIMD_HIP_OK) return rc;
  if (n != 0 && any_alias({r, s_, px}, {d, aux, msg})) return bad(ctx, "r, s and px must not alias an input or each other");
  ENTER_ANY_SIZE();
  const int curve = ECSIMD_HIP_SECP256K1;
  const size_t chunk = chunk_of(n, GC_CHUNK);
  jacobian j; uint64_t *xP = nullptr, *yP = nullptr, *xR = nullptr, *yR = nullptr, *k0 = nullptr;
  auto place = [&](void* base) {
    carve c = carve_from(base);
    j = carve_jacobian(c, chunk); xP = carve_limbs(c, chunk); yP = carve_limbs(c, chunk); xR = carve_limbs(c, chunk); yR = carve_limbs(c, chunk); k0 = carve_limbs(c, chunk);
    return c;
  };
  rc = ensure_window_table(ctx, curve, CT_WBITS);
  if (rc == ECSIMD_HIP_OK) rc = ensure_workspace(ctx, place(nullptr).bytes);
  if (rc != ECSIMD_HIP_OK) return rc;
  const carve ws = place(ctx->workspace);
  hipStream_t st = ctx->stream;
  hipError_t err = hipSuccess;
  FOR_CHUNKS(first, m, n, chunk) {
    const uint8_t* mp = msg ? msg + first * stride_bytes : nullptr;
    secret_base_product(ctx, curve, d + 4 * first, j, xP, yP, m);
    launch::schnorr_nonce(st, O.words, d + 4 * first, aux ? aux + 4 * first : nullptr, xP, yP, mp, msg_bytes, stride_bytes, k0, m);
    secret_base_product(ctx, curve, k0, j, xR, yR, m);
    launch::schnorr_finish(st, O.N, d + 4 * first, k0, xP, yP, xR, yR, mp, msg_bytes, stride_bytes, px ? px + 4 * first : nullptr, r + 4 * first, s_ + 4 * first, ok + first, m);
    err = wipe_workspace(ctx, ws.bytes, hipGetLastError());
    if (err != hipSuccess) break;
  }
  return err == hipSuccess ? ECSIMD_HIP_OK : fail(ctx, err, "schnorr_sign launch"); }

// ---- Ed25519 (include/ecsimd_ed25519.h; k_ed25519.hip).  Bytes in, bytes out; the multiples of B are constants of the library, so nothing is built at run time
// and the only thing a capture can refuse is a workspace that would have to grow.  ECSIMD_HIP_REF_SQUARE_COMPAT contexts are accepted: none of the reference's
// arithmetic is involved.
namespace {
// L = 2^252 + 27742317777372353535851937790883648493 as the scalar kernels take it
const gmod* ed25519_order() {
  static const uint64_t l[4] = {0x5812631a5cf5d3edull, 0x14def9dea2f79cd6ull, 0x0000000000000000ull, 0x1000000000000000ull};
  static const gmod M = make_gmod(l, GMOD_PRIME);
  return &M;
}
// keccak256's message arguments, checked the same way; msg_bytes comes back as 0 where lens rules
int ed25519_messages(ecsimd_hip_ctx* ctx, const uint8_t* msg, size_t* msg_bytes, size_t stride_bytes, const uint32_t* lens, size_t n) {
  if (lens) *msg_bytes = 0;
  if (!msg && n && (*msg_bytes || (lens && stride_bytes))) return bad(ctx, "msg is null");
  if (lens && (reinterpret_cast<uintptr_t>(lens) & 3u)) return bad(ctx, "lens is not 4-byte aligned");
  if (stride_bytes < *msg_bytes) return bad(ctx, "ed25519: stride_bytes is smaller than msg_bytes");
  if (*msg_bytes > ((size_t)1 << 40)) return bad(ctx, "ed25519: message too long");
  return ECSIMD_HIP_OK;
}
// Per lane of a chunk: the scalars a and r side by side (one comb launch takes both), then their encodings the same way.  pubkey needs a alone.
struct ed25519_secret_layout { uint64_t *a, *r; uint8_t *encA, *encR; size_t bytes; };
ed25519_secret_layout ed25519_secret_plan(void* base, size_t chunk, bool sign) {
  ed25519_secret_layout L; carve c = carve_from(base);
  L.a = carve_limbs(c, chunk); L.r = sign ? carve_limbs(c, chunk) : nullptr;
  L.encA = sign ? static_cast<uint8_t*>(carve_bytes(c, 32 * chunk)) : nullptr; L.encR = sign ? static_cast<uint8_t*>(carve_bytes(c, 32 * chunk)) : nullptr;
  L.bytes = c.bytes;
  return L;
}
// The longest launch is the verification loop's: 2^20 lanes of it stay within what DESIGN.md section 4d allows a launch on a shared device, and 1 KiB of
// table per lane keeps the workspace at 1.1 GB.
constexpr size_t ED25519_VERIFY_CHUNK = (size_t)1 << 20;
struct ed25519_verify_layout { uint64_t *s, *h; void* table; uint8_t* valid; size_t bytes; };
ed25519_verify_layout ed25519_verify_plan(void* base, size_t chunk) {
  ed25519_verify_layout L; carve c = carve_from(base);
  L.s = carve_limbs(c, chunk); L.h = carve_limbs(c, chunk); L.table = carve_bytes(c, launch::ed25519_table_bytes(chunk)); L.valid = carve_flags(c, chunk);
  L.bytes = c.bytes;
  return L;
}
}  // namespace

int ecsimd_ed25519_pubkey(ecsimd_hip_ctx* ctx, const uint8_t* seed, uint8_t* pk, size_t n) {
  REQUIRE_CTX(); if ((!seed || !pk) && n) return bad(ctx, "ed25519_pubkey: seed or pk is null");
  if (n != 0 && overlaps(seed, pk)) return bad(ctx, "ed25519_pubkey: pk must not alias seed");
  ENTER_ANY_SIZE();
  const size_t chunk = chunk_of(n, GC_CHUNK);
  int rc = ensure_workspace(ctx, ed25519_secret_plan(nullptr, chunk, false).bytes);
  if (rc != ECSIMD_HIP_OK) return rc;
  const ed25519_secret_layout L = ed25519_secret_plan(ctx->workspace, chunk, false);
  hipError_t err = hipSuccess;
  FOR_CHUNKS(first, m, n, chunk) {
    launch::ed25519_secret_front(ctx->stream, *ed25519_order(), seed + 32 * first, nullptr, 0, 0, nullptr, false, L.a, nullptr, m);
    launch::ed25519_base_ct(ctx->stream, L.a, pk + 32 * first, m);
    err = wipe_workspace(ctx, L.bytes, hipGetLastError());
    if (err != hipSuccess) break;
  }
  return err == hipSuccess ? ECSIMD_HIP_OK : fail(ctx, err, "ed25519_pubkey launch"); }

int ecsimd_ed25519_sign(ecsimd_hip_ctx* ctx, const uint8_t* seed, const uint8_t* msg, size_t msg_bytes, size_t stride_bytes, const uint32_t* lens,
                        uint8_t* sig, uint8_t* pk, size_t n) {
  REQUIRE_CTX(); if ((!seed || !sig) && n) return bad(ctx, "ed25519_sign: seed or sig is null");
  int rc = ed25519_messages(ctx, msg, &msg_bytes, stride_bytes, lens, n); if (rc != ECSIMD_HIP_OK) return rc;
  if (n != 0 && (pk ? any_alias({sig, pk}, {seed, msg, lens}) : any_alias({sig}, {seed, msg, lens}))) return bad(ctx, "ed25519_sign: sig and pk must not alias an input or each other");
  ENTER_ANY_SIZE();
  const size_t chunk = chunk_of(n, GC_CHUNK);
  rc = ensure_workspace(ctx, ed25519_secret_plan(nullptr, chunk, true).bytes);
  if (rc != ECSIMD_HIP_OK) return rc;
  const ed25519_secret_layout L = ed25519_secret_plan(ctx->workspace, chunk, true);
  hipError_t err = hipSuccess;
  FOR_CHUNKS(first, m, n, chunk) {
    const uint8_t* mp = msg ? msg + first * stride_bytes : nullptr;
    const uint32_t* lp = lens ? lens + first : nullptr;
    launch::ed25519_secret_front(ctx->stream, *ed25519_order(), seed + 32 * first, mp, msg_bytes, stride_bytes, lp, true, L.a, L.r, m);
    // a and r lie `chunk` lanes apart, and so do their encodings: a full chunk takes one comb launch of 2 m lanes, a shorter one two
    if (m == chunk) launch::ed25519_base_ct(ctx->stream, L.a, L.encA, 2 * m);
    else { launch::ed25519_base_ct(ctx->stream, L.a, L.encA, m); launch::ed25519_base_ct(ctx->stream, L.r, L.encR, m); }
    launch::ed25519_sign_finish(ctx->stream, *ed25519_order(), L.a, L.r, L.encA, L.encR, mp, msg_bytes, stride_bytes, lp, sig + 64 * first, pk ? pk + 32 * first : nullptr, m);
    err = wipe_workspace(ctx, L.bytes, hipGetLastError());
    if (err != hipSuccess) break;
  }
  return err == hipSuccess ? ECSIMD_HIP_OK : fail(ctx, err, "ed25519_sign launch"); }

int ecsimd_ed25519_verify(ecsimd_hip_ctx* ctx, const uint8_t* pk, const uint8_t* msg, size_t msg_bytes, size_t stride_bytes, const uint32_t* lens,
                          const uint8_t* sig, uint8_t* ok, size_t n, int flags) {
  REQUIRE_CTX(); if ((!pk || !sig || !ok) && n) return bad(ctx, "ed25519_verify: pk, sig or ok is null");
  if (flags & ~ECSIMD_ED25519_REJECT_SMALL_ORDER) return bad(ctx, "ed25519_verify: unknown flag");
  int rc = ed25519_messages(ctx, msg, &msg_bytes, stride_bytes, lens, n); if (rc != ECSIMD_HIP_OK) return rc;
  if (n != 0 && any_alias({ok}, {pk, msg, sig, lens})) return bad(ctx, "ed25519_verify: ok must not alias an input");
  ENTER_ANY_SIZE();
  const size_t chunk = chunk_of(n, ED25519_VERIFY_CHUNK);
  rc = ensure_workspace(ctx, ed25519_verify_plan(nullptr, chunk).bytes);
  if (rc != ECSIMD_HIP_OK) return rc;
  const ed25519_verify_layout L = ed25519_verify_plan(ctx->workspace, chunk);
  FOR_CHUNKS(first, m, n, chunk) {
    launch::ed25519_verify_front(ctx->stream, *ed25519_order(), pk + 32 * first, sig + 64 * first, msg ? msg + first * stride_bytes : nullptr, msg_bytes, stride_bytes,
                                 lens ? lens + first : nullptr, (flags & ECSIMD_ED25519_REJECT_SMALL_ORDER) != 0, L.s, L.h, L.table, L.valid, m);
    launch::ed25519_verify_loop(ctx->stream, L.s, L.h, L.table, L.valid, sig + 64 * first, ok + first, m);
  }
  const hipError_t err = hipGetLastError();
  return err == hipSuccess ? ECSIMD_HIP_OK : fail(ctx, err, "ed25519_verify launch"); }

int ecsimd_ed25519_raw_inputs(int op) { return (op < 0 || op > launch::ED_RAW_DOUBLE_MULT) ? 0 : launch::ed_raw_inputs(op); }
int ecsimd_ed25519_raw_outputs(int op) { return (op < 0 || op > launch::ED_RAW_DOUBLE_MULT) ? 0 : launch::ed_raw_outputs(op); }
int ecsimd_ed25519_raw(ecsimd_hip_ctx* ctx, int op, const uint8_t* in, uint8_t* out, size_t n) {
  REQUIRE_CTX(); if ((!in || !out) && n) return bad(ctx, "ed25519_raw: null pointer");
  if (op < 0 || op > launch::ED_RAW_DOUBLE_MULT) return bad(ctx, "ed25519_raw: unknown function");
  if (n != 0 && overlaps(in, out)) return bad(ctx, "ed25519_raw: out must not alias in");
  ENTER();
  void* table = nullptr;
  if (op == launch::ED_RAW_DOUBLE_MULT) {
    if (n > ED25519_VERIFY_CHUNK) return bad(ctx, "ed25519_raw: at most 2^20 lanes of DOUBLE_MULT");
    const int rc = ensure_workspace(ctx, launch::ed25519_table_bytes(n));
    if (rc != ECSIMD_HIP_OK) return rc;
    table = ctx->workspace;
  }
  launch::ed25519_raw(ctx->stream, *ed25519_order(), op, in, out, table, n);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? ECSIMD_HIP_OK : fail(ctx, e, "ed25519_raw launch"); }

// ---- X25519 and the Ed25519 key conversions (include/ecsimd_x25519.h; k_x25519.hip).  Bytes in, bytes out, one kernel per call and no workspace: nothing to
// size, nothing to wipe, nothing a capture can refuse.  ECSIMD_HIP_REF_SQUARE_COMPAT contexts are accepted: none of the reference's arithmetic is involved.
namespace {
// One launch covers at most 2^20 lanes (ed25519_verify's figure): the ladder is the longest kernel here, and DESIGN.md section 4g has what a launch of it takes.
constexpr size_t X25519_CHUNK = (size_t)1 << 20;
}  // namespace

int ecsimd_x25519(ecsimd_hip_ctx* ctx, const uint8_t* scalar, const uint8_t* u, uint8_t* out, uint8_t* ok, size_t n) {
  REQUIRE_CTX(); if ((!scalar || !u || !out) && n) return bad(ctx, "x25519: scalar, u or out is null");
  if (n != 0 && (ok ? any_alias({out, ok}, {scalar, u}) : any_alias({out}, {scalar, u}))) return bad(ctx, "x25519: out and ok must not alias an input or each other");
  ENTER_ANY_SIZE();
  FOR_CHUNKS(first, m, n, X25519_CHUNK) launch::x25519(ctx->stream, scalar + 32 * first, u + 32 * first, out + 32 * first, ok ? ok + first : nullptr, m);
  const hipError_t err = hipGetLastError();
  return err == hipSuccess ? ECSIMD_HIP_OK : fail(ctx, err, "x25519 launch"); }

int ecsimd_x25519_base(ecsimd_hip_ctx* ctx, const uint8_t* scalar, uint8_t* out, size_t n) {
  REQUIRE_CTX(); if ((!scalar || !out) && n) return bad(ctx, "x25519_base: scalar or out is null");
  if (n != 0 && overlaps(scalar, out)) return bad(ctx, "x25519_base: out must not alias scalar");
  ENTER_ANY_SIZE();
  FOR_CHUNKS(first, m, n, X25519_CHUNK) launch::x25519_base(ctx->stream, *ed25519_order(), scalar + 32 * first, out + 32 * first, m);
  const hipError_t err = hipGetLastError();
  return err == hipSuccess ? ECSIMD_HIP_OK : fail(ctx, err, "x25519_base launch"); }

int ecsimd_x25519_from_ed25519_pk(ecsimd_hip_ctx* ctx, const uint8_t* pk, uint8_t* u, uint8_t* ok, size_t n) {
  REQUIRE_CTX(); if ((!pk || !u || !ok) && n) return bad(ctx, "x25519_from_ed25519_pk: pk, u or ok is null");
  if (n != 0 && any_alias({u, ok}, {pk})) return bad(ctx, "x25519_from_ed25519_pk: u and ok must not alias an input or each other");
  ENTER_ANY_SIZE();
  FOR_CHUNKS(first, m, n, X25519_CHUNK) launch::x25519_from_ed_pk(ctx->stream, pk + 32 * first, u + 32 * first, ok + first, m);
  const hipError_t err = hipGetLastError();
  return err == hipSuccess ? ECSIMD_HIP_OK : fail(ctx, err, "x25519_from_ed25519_pk launch"); }

int ecsimd_x25519_from_ed25519_seed(ecsimd_hip_ctx* ctx, const uint8_t* seed, uint8_t* scalar, size_t n) {
  REQUIRE_CTX(); if ((!seed || !scalar) && n) return bad(ctx, "x25519_from_ed25519_seed: seed or scalar is null");
  if (n != 0 && overlaps(seed, scalar)) return bad(ctx, "x25519_from_ed25519_seed: scalar must not alias seed");
  ENTER_ANY_SIZE();
  FOR_CHUNKS(first, m, n, X25519_CHUNK) launch::x25519_from_ed_seed(ctx->stream, seed + 32 * first, scalar + 32 * first, m);
  const hipError_t err = hipGetLastError();
  return err == hipSuccess ? ECSIMD_HIP_OK : fail(ctx, err, "x25519_from_ed25519_seed launch"); }

int ecsimd_x25519_raw_inputs(int op) { return (op < 0 || op > launch::X25519_RAW_ED_TO_MONT) ? 0 : launch::x25519_raw_inputs(op); }
int ecsimd_x25519_raw_outputs(int op) { return (op < 0 || op > launch::X25519_RAW_ED_TO_MONT) ? 0 : launch::x25519_raw_outputs(op); }
int ecsimd_x25519_raw(ecsimd_hip_ctx* ctx, int op, const uint8_t* in, uint8_t* out, size_t n) {
  REQUIRE_CTX(); if ((!in || !out) && n) return bad(ctx, "x25519_raw: null pointer");
  if (op < 0 || op > launch::X25519_RAW_ED_TO_MONT) return bad(ctx, "x25519_raw: unknown function");
  if (n != 0 && overlaps(in, out)) return bad(ctx, "x25519_raw: out must not alias in");
  ENTER_ANY_SIZE();
  const size_t ni = launch::x25519_raw_inputs(op), no = launch::x25519_raw_outputs(op);
  FOR_CHUNKS(first, m, n, X25519_CHUNK) launch::x25519_raw(ctx->stream, op, in + 32 * ni * first, out + 32 * no * first, m);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? ECSIMD_HIP_OK : fail(ctx, e, "x25519_raw launch"); }

// ---- NIST P-384 (include/ecsimd_p384.h; k_p384.hip).  Bytes in, bytes out; the multiples of G are constants of the library, so nothing is built at run time
// and the only thing a capture can refuse is a workspace that would have to grow.  ECSIMD_HIP_REF_SQUARE_COMPAT contexts are accepted: none of the reference's
// arithmetic is involved.
namespace {
// One launch covers at most 2^16 lanes: the kernels hold a twelve-word point law in registers and run one wave per SIMD, so 2^16 lanes are one full round of
// the device, a launch of the longest of them (verification) stays short on a shared device, and the lanes' tables take 75 MB of workspace.
constexpr size_t P384_CHUNK = (size_t)1 << 16;
struct p384_table_layout { uint32_t* table; size_t bytes; };
p384_table_layout p384_table_plan(void* base, size_t chunk) {
  p384_table_layout L; carve c = carve_from(base);
  L.table = static_cast<uint32_t*>(carve_bytes(c, launch::p384_table_bytes(chunk)));
  L.bytes = c.bytes;
  return L;
}
struct p384_sign_layout { uint32_t* kws; size_t bytes; };
p384_sign_layout p384_sign_plan(void* base, size_t chunk) {
  p384_sign_layout L; carve c = carve_from(base);
  L.kws = static_cast<uint32_t*>(carve_bytes(c, launch::p384_nonce_bytes(chunk)));
  L.bytes = c.bytes;
  return L;
}
}  // namespace

int ecsimd_p384_sha384(ecsimd_hip_ctx* ctx, const uint8_t* msg, size_t msg_bytes, size_t stride_bytes, const uint32_t* lens, uint8_t* digest, size_t n) {
  REQUIRE_CTX(); if (!digest && n) return bad(ctx, "p384_sha384: digest is null");
  int rc = ed25519_messages(ctx, msg, &msg_bytes, stride_bytes, lens, n); if (rc != ECSIMD_HIP_OK) return rc;
  if (n != 0 && any_alias({digest}, {msg, lens})) return bad(ctx, "p384_sha384: digest must not alias an input");
  ENTER_ANY_SIZE();
  FOR_CHUNKS(first, m, n, P384_CHUNK)
    launch::p384_sha384(ctx->stream, msg ? msg + first * stride_bytes : nullptr, msg_bytes, stride_bytes, lens ? lens + first : nullptr, digest + 48 * first, m);
  const hipError_t err = hipGetLastError();
  return err == hipSuccess ? ECSIMD_HIP_OK : fail(ctx, err, "p384_sha384 launch"); }

int ecsimd_p384_pubkey(ecsimd_hip_ctx* ctx, const uint8_t* d, uint8_t* pub, uint8_t* ok, size_t n) {
  REQUIRE_CTX(); if ((!d || !pub || !ok) && n) return bad(ctx, "p384_pubkey: d, pub or ok is null");
  if (n != 0 && any_alias({pub, ok}, {d})) return bad(ctx, "p384_pubkey: pub and ok must not alias an input or each other");
  ENTER_ANY_SIZE();
  FOR_CHUNKS(first, m, n, P384_CHUNK) launch::p384_pubkey(ctx->stream, d + 48 * first, pub + 96 * first, ok + first, m);
  const hipError_t err = hipGetLastError();
  return err == hipSuccess ? ECSIMD_HIP_OK : fail(ctx, err, "p384_pubkey launch"); }

int ecsimd_p384_ecdh(ecsimd_hip_ctx* ctx, const uint8_t* d, const uint8_t* peer, uint8_t* z, uint8_t* ok, size_t n) {
  REQUIRE_CTX(); if ((!d || !peer || !z || !ok) && n) return bad(ctx, "p384_ecdh: d, peer, z or ok is null");
  if (n != 0 && any_alias({z, ok}, {d, peer})) return bad(ctx, "p384_ecdh: z and ok must not alias an input or each other");
  ENTER_ANY_SIZE();
  const size_t chunk = chunk_of(n, P384_CHUNK);
  const int rc = ensure_workspace(ctx, p384_table_plan(nullptr, chunk).bytes);
  if (rc != ECSIMD_HIP_OK) return rc;
  const p384_table_layout L = p384_table_plan(ctx->workspace, chunk);
  hipError_t err = hipSuccess;
  FOR_CHUNKS(first, m, n, chunk) {
    launch::p384_ecdh(ctx->stream, d + 48 * first, peer + 96 * first, L.table, z + 48 * first, ok + first, m);
    err = wipe_workspace(ctx, L.bytes, hipGetLastError());        // multiples of the public peer: wiped all the same, no value of a secret call stays behind
    if (err != hipSuccess) break;
  }
  return err == hipSuccess ? ECSIMD_HIP_OK : fail(ctx, err, "p384_ecdh launch"); }

int ecsimd_p384_ecdsa_verify(ecsimd_hip_ctx* ctx, const uint8_t* pub, const uint8_t* digest, const uint8_t* sig, uint8_t* ok, size_t n) {
  REQUIRE_CTX(); if ((!pub || !digest || !sig || !ok) && n) return bad(ctx, "p384_ecdsa_verify: pub, digest, sig or ok is null");
  if (n != 0 && any_alias({ok}, {pub, digest, sig})) return bad(ctx, "p384_ecdsa_verify: ok must not alias an input");
  ENTER_ANY_SIZE();
  const size_t chunk = chunk_of(n, P384_CHUNK);
  const int rc = ensure_workspace(ctx, p384_table_plan(nullptr, chunk).bytes);
  if (rc != ECSIMD_HIP_OK) return rc;
  const p384_table_layout L = p384_table_plan(ctx->workspace, chunk);
  FOR_CHUNKS(first, m, n, chunk) launch::p384_verify(ctx->stream, pub + 96 * first, digest + 48 * first, sig + 96 * first, L.table, ok + first, m);
  const hipError_t err = hipGetLastError();
  return err == hipSuccess ? ECSIMD_HIP_OK : fail(ctx, err, "p384_ecdsa_verify launch"); }

int ecsimd_p384_ecdsa_sign(ecsimd_hip_ctx* ctx, const uint8_t* d, const uint8_t* digest, uint8_t* sig, uint8_t* ok, size_t n, int flags) {
  REQUIRE_CTX(); if ((!d || !digest || !sig || !ok) && n) return bad(ctx, "p384_ecdsa_sign: d, digest, sig or ok is null");
  if (flags != 0) return bad(ctx, "p384_ecdsa_sign: flags must be 0");
  if (n != 0 && any_alias({sig, ok}, {d, digest})) return bad(ctx, "p384_ecdsa_sign: sig and ok must not alias an input or each other");
  ENTER_ANY_SIZE();
  const size_t chunk = chunk_of(n, P384_CHUNK);
  const int rc = ensure_workspace(ctx, p384_sign_plan(nullptr, chunk).bytes);
  if (rc != ECSIMD_HIP_OK) return rc;
  const p384_sign_layout L = p384_sign_plan(ctx->workspace, chunk);
  hipError_t err = hipSuccess;
  FOR_CHUNKS(first, m, n, chunk) {
    launch::p384_sign_nonce(ctx->stream, d + 48 * first, digest + 48 * first, L.kws, m);
    launch::p384_sign_finish(ctx->stream, d + 48 * first, digest + 48 * first, L.kws, sig + 96 * first, ok + first, m);
    err = wipe_workspace(ctx, L.bytes, hipGetLastError());        // k and its validity; K, V, k G and its inverse never leave the registers
    if (err != hipSuccess) break;
  }
  return err == hipSuccess ? ECSIMD_HIP_OK : fail(ctx, err, "p384_ecdsa_sign launch"); }

int ecsimd_p384_raw_inputs(int op) { return (op < 0 || op > launch::P384_RAW_DOUBLE_MULT) ? 0 : launch::p384_raw_inputs(op); }
int ecsimd_p384_raw_outputs(int op) { return (op < 0 || op > launch::P384_RAW_DOUBLE_MULT) ? 0 : launch::p384_raw_outputs(op); }
int ecsimd_p384_raw(ecsimd_hip_ctx* ctx, int op, const uint8_t* in, uint8_t* out, size_t n) {
  REQUIRE_CTX(); if ((!in || !out) && n) return bad(ctx, "p384_raw: null pointer");
  if (op < 0 || op > launch::P384_RAW_DOUBLE_MULT) return bad(ctx, "p384_raw: unknown function");
  if (n != 0 && overlaps(in, out)) return bad(ctx, "p384_raw: out must not alias in");
  ENTER();
  uint32_t* table = nullptr;
  if (op == launch::P384_RAW_VAR_MULT || op == launch::P384_RAW_DOUBLE_MULT) {
    if (n > P384_CHUNK) return bad(ctx, "p384_raw: at most 2^16 lanes of VAR_MULT and DOUBLE_MULT");
    const int rc = ensure_workspace(ctx, p384_table_plan(nullptr, n).bytes);
    if (rc != ECSIMD_HIP_OK) return rc;
    table = p384_table_plan(ctx->workspace, n).table;
  }
  launch::p384_raw(ctx->stream, op, in, out, table, n);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? ECSIMD_HIP_OK : fail(ctx, e, "p384_raw launch"); }

// ---- The SM2 signature scheme on a registered curve with the ECDSA capability (include/ecsimd_sm2.h; k_sm2.hip): SM3, Z_A and the scalar-field halves are new
// kernels, launched once over the whole batch; every point is made by the steps ECDSA uses on such a curve -- gc_double_scalar_mult for the public sum
// s G + t Q, the constant-time comb of ecdsa_sign_registered for the secret k G and d G -- and signing's workspace goes through wipe_workspace.
namespace {
int sm2_require(ecsimd_hip_ctx* ctx, int curve, curve_record* rec) {
  if (curve == ECSIMD_HIP_P256 || curve == ECSIMD_HIP_SECP256K1)
    return bad(ctx, "sm2: a curve registered at run time with the ECDSA capability is needed (ecsimd_sm2_curve gives sm2p256v1's id): the built-in curve ids are refused");
  return gc_require_ecdsa(ctx, curve, rec);
}
launch::sm2_curve_words sm2_words(const curve_record& rec) {
  launch::sm2_curve_words w;
  w.a = words8_of(rec.a.l); w.b = words8_of(rec.b.l);
  for (int i = 0; i < 8; ++i) { w.gx.w[i] = rec.G.gx[i]; w.gy.w[i] = rec.G.gy[i]; }
  return w;
}
int sm2_id_args(ecsimd_hip_ctx* ctx, const uint8_t* id, size_t id_bytes, size_t id_stride, size_t n) {
  if (id_bytes > 8191) return bad(ctx, "sm2: id_bytes is larger than 8191 (ENTL, the identity's bit length, has 16 bits)");
  if (!id && n && id_bytes) return bad(ctx, "sm2: id is null");
  if (id_stride != 0 && id_stride < id_bytes) return bad(ctx, "sm2: id_stride is smaller than id_bytes (0: one identity for the whole batch)");
  return ECSIMD_HIP_OK;
}
int sm2_msg_args(ecsimd_hip_ctx* ctx, const uint8_t* msg, size_t* msg_bytes, size_t stride_bytes, const uint32_t* lens, size_t n) {
  if (lens) *msg_bytes = 0;                                                       // (ignored: every lane has its own length)
  if (!msg && n && (*msg_bytes || (lens && stride_bytes))) return bad(ctx, "sm2: msg is null");
  if (lens && (reinterpret_cast<uintptr_t>(lens) & 3u)) return bad(ctx, "sm2: lens is not 4-byte aligned");
  if (lens && !stride_bytes && n > 1) return bad(ctx, "sm2: stride_bytes is 0 with lens: every lane would read the first row");
  if (stride_bytes < *msg_bytes) return bad(ctx, "sm2: stride_bytes is smaller than msg_bytes");
  if (*msg_bytes >= ((size_t)1 << 31)) return bad(ctx, "sm2: message too long (2^31 bytes or more)");
  return ECSIMD_HIP_OK;
}
// verification's own arrays behind the double product's and verify_plan's: u1 = s, u2 = t, the digest where the call makes it, the range flags
struct sm2_verify_layout { uint64_t *u1, *u2, *e; uint8_t* valid; size_t extra; };
sm2_verify_layout sm2_verify_plan(void* base, size_t front, size_t n, bool with_e) {
  sm2_verify_layout S; carve c = carve_from(base);
  (void)carve_bytes(c, front); S.u1 = carve_limbs(c, n); S.u2 = carve_limbs(c, n); S.e = with_e ? carve_limbs(c, n) : nullptr; S.valid = carve_flags(c, n); S.extra = c.bytes - front;
  return S;
}
// msg_of == nullptr: the caller's digest e.  Else e = SM3(Z_A || M) into the workspace first.  The caller has gone through ENTER.
struct sm2_message { const uint8_t* id; size_t id_bytes, id_stride; const uint8_t* msg; size_t msg_bytes, stride_bytes; const uint32_t* lens; };
int sm2_verify_impl(ecsimd_hip_ctx* ctx, int curve, const curve_record& rec, const uint64_t* e, const sm2_message* msg_of, const uint64_t* r, const uint64_t* s_, const uint64_t* qx,
                    const uint64_t* qy, uint8_t* ok, size_t n) {
  const size_t front = gc_plan(nullptr, n, gc_window_possible(rec)).bytes, behind = verify_plan(nullptr, front, n).behind, inner = front + behind;
  int rc = ensure_workspace(ctx, inner + sm2_verify_plan(nullptr, inner, n, msg_of != nullptr).extra);
  if (rc != ECSIMD_HIP_OK) return rc;
  const sm2_verify_layout S = sm2_verify_plan(ctx->workspace, inner, n, msg_of != nullptr);
  const verify_layout V = verify_plan(ctx->workspace, front, n);
  if (msg_of) {
    launch::sm2_digest(ctx->stream, sm2_words(rec), qx, qy, msg_of->id, msg_of->id_bytes, msg_of->id_stride, msg_of->msg, msg_of->msg_bytes, msg_of->stride_bytes, msg_of->lens, S.e, n);
    e = S.e;
  }
  launch::sm2_verify_scalars(ctx->stream, order_words(rec), r, s_, S.u1, S.u2, S.valid, n);
  rc = gc_double_scalar_mult(ctx, curve, rec, S.u1, S.u2, qx, qy, V.rx, nullptr, V.fin, n, behind + S.extra);      // the workspace is already this large: nothing moves
  if (rc != ECSIMD_HIP_OK) return rc;
  launch::sm2_accept(ctx->stream, order_words(rec), e, V.rx, V.fin, r, S.valid, ok, n);                            // fin is 0 for the lanes whose Q failed validation
  const hipError_t err = hipGetLastError();
  return err == hipSuccess ? ECSIMD_HIP_OK : fail(ctx, err, "sm2_verify launch");
}
// k G for SECRET k on the registered curve, x (and y) affine into the caller's arrays: ecdsa_sign_registered's product -- the constant-time 5-bit comb of the
// generator; where no table exists yet and a capture in progress forbids building it, the reference's ladder, constant-time as it is.  L's arrays are the
// caller's to wipe.  ensure_sm2_comb comes first: it may synchronise, and runs before any pointer into the workspace is taken.
int ensure_sm2_comb(ecsimd_hip_ctx* ctx, int curve, const curve_record& rec, const uint32_t** comb) {
  *comb = nullptr;
  if (!gc_comb_possible(rec)) return ECSIMD_HIP_OK;
  const int rc = ensure_gc_comb(ctx, curve, rec, comb, 5);
  if (rc != ECSIMD_HIP_OK) { if (!capturing(ctx)) return rc; *comb = nullptr; }
  return ECSIMD_HIP_OK;
}
void sm2_secret_product(ecsimd_hip_ctx* ctx, const curve_record& rec, const gc_layout& L, const uint32_t* comb, const uint64_t* k, uint64_t* x, uint64_t* y, size_t n) {
  if (comb) {
    launch::gc_base_windowed_s(ctx->stream, rec.G, order_words(rec), 5, k, comb, L.j[0], L.j[1], L.j[2], n);      // k >= n is reduced by the comb; the caller's kernel refuses the lane
    launch::gc_to_affine_batched(ctx->stream, rec.G, L.j[0], L.j[1], L.j[2], x, y, n);
  } else gc_safe_mult(ctx->stream, rec, L, L.adj1, L.neg1, k, nullptr, nullptr, x, y, n);
}
// signing's workspace: the product's arrays, then (deterministic nonce) the nonce, K, V and the retry bytes
struct sm2_sign_layout { gc_layout G; nonce_layout K; size_t bytes; };
sm2_sign_layout sm2_sign_plan(uint64_t* base, size_t n, bool nonce) {
  sm2_sign_layout L; L.G = gc_plan(base, n);
  L.K = nonce_plan_ws(base, L.G.bytes, nonce ? n : 0);
  L.bytes = L.G.bytes + (nonce ? L.K.bytes : 0);
  return L;
}
const uint64_t SM2P256V1[6][4] = {
    {0xffffffffffffffffull, 0xffffffff00000000ull, 0xffffffffffffffffull, 0xfffffffeffffffffull},      // p
    {0xfffffffffffffffcull, 0xffffffff00000000ull, 0xffffffffffffffffull, 0xfffffffeffffffffull},      // a = p - 3
    {0xddbcbd414d940e93ull, 0xf39789f515ab8f92ull, 0x4d5a9e4bcf6509a7ull, 0x28e9fa9e9d9f5e34ull},      // b
    {0x715a4589334c74c7ull, 0x8fe30bbff2660be1ull, 0x5f9904466a39c994ull, 0x32c4ae2c1f198119ull},      // x_G
    {0x02df32e52139f0a0ull, 0xd0a9877cc62a4740ull, 0x59bdcee36b692153ull, 0xbc3736a2f4f6779cull},      // y_G
    {0x53bbf40939d54123ull, 0x7203df6b21c6052bull, 0xffffffffffffffffull, 0xfffffffeffffffffull}};     // n
}  // namespace

int ecsimd_sm2_curve(int* curve_id) {
  if (!curve_id) return ECSIMD_HIP_ERR_BAD_ARG;
  return ecsimd_hip_register_curve(SM2P256V1[0], SM2P256V1[1], SM2P256V1[2], SM2P256V1[3], SM2P256V1[4], SM2P256V1[5], 0, curve_id); }

int ecsimd_sm2_sm3(ecsimd_hip_ctx* ctx, const uint8_t* msg, size_t msg_bytes, size_t stride_bytes, const uint32_t* lens, uint64_t* e, size_t n) {
  REQUIRE_CTX(); REQUIRE_PTR(e);
  int rc = sm2_msg_args(ctx, msg, &msg_bytes, stride_bytes, lens, n); if (rc != ECSIMD_HIP_OK) return rc;
  if (n != 0 && any_alias({e}, {msg, lens})) return bad(ctx, "sm2_sm3: e must not alias an input");
  RUN(launch::sm3(s, msg, msg_bytes, stride_bytes, lens, e, n)); }

int ecsimd_sm2_za(ecsimd_hip_ctx* ctx, int curve, const uint64_t* qx, const uint64_t* qy, const uint8_t* id, size_t id_bytes, size_t id_stride, uint64_t* za, size_t n) {
  REQUIRE_CTX(); REQUIRE_PTR(qx); REQUIRE_PTR(qy); REQUIRE_PTR(za);
  curve_record rec; int rc = sm2_require(ctx, curve, &rec); if (rc != ECSIMD_HIP_OK) return rc;
  rc = sm2_id_args(ctx, id, id_bytes, id_stride, n); if (rc != ECSIMD_HIP_OK) return rc;
  if (n != 0 && any_alias({za}, {qx, qy, id})) return bad(ctx, "sm2_za: za must not alias an input");
  RUN(launch::sm2_za(s, sm2_words(rec), qx, qy, id, id_bytes, id_stride, za, n)); }

int ecsimd_sm2_digest(ecsimd_hip_ctx* ctx, int curve, const uint64_t* qx, const uint64_t* qy, const uint8_t* id, size_t id_bytes, size_t id_stride, const uint8_t* msg,
                      size_t msg_bytes, size_t stride_bytes, const uint32_t* lens, uint64_t* e, size_t n) {
  REQUIRE_CTX(); REQUIRE_PTR(qx); REQUIRE_PTR(qy); REQUIRE_PTR(e);
  curve_record rec; int rc = sm2_require(ctx, curve, &rec); if (rc != ECSIMD_HIP_OK) return rc;
  rc = sm2_id_args(ctx, id, id_bytes, id_stride, n); if (rc != ECSIMD_HIP_OK) return rc;
  rc = sm2_msg_args(ctx, msg, &msg_bytes, stride_bytes, lens, n); if (rc != ECSIMD_HIP_OK) return rc;
  if (n != 0 && any_alias({e}, {qx, qy, id, msg, lens})) return bad(ctx, "sm2_digest: e must not alias an input");
  RUN(launch::sm2_digest(s, sm2_words(rec), qx, qy, id, id_bytes, id_stride, msg, msg_bytes, stride_bytes, lens, e, n)); }

int ecsimd_sm2_pubkey(ecsimd_hip_ctx* ctx, int curve, const uint64_t* d, uint64_t* qx, uint64_t* qy, uint8_t* ok, size_t n) {
  REQUIRE_CTX(); REQUIRE_PTR(d); REQUIRE_PTR(qx); REQUIRE_PTR(qy);
  if (!ok && n) return bad(ctx, "ok is null");
  curve_record rec; int rc = sm2_require(ctx, curve, &rec); if (rc != ECSIMD_HIP_OK) return rc;
  if (n != 0 && any_alias({qx, qy, ok}, {d})) return bad(ctx, "sm2_pubkey: qx, qy and ok must not alias an input or each other");
  ENTER();
  if (gc_plan(nullptr, n).chunk != n) return bad(ctx, "sm2_pubkey: at most 2^22 keys per call");
  rc = ensure_workspace(ctx, gc_plan(nullptr, n).bytes);
  if (rc != ECSIMD_HIP_OK) return rc;
  const uint32_t* comb; rc = ensure_sm2_comb(ctx, curve, rec, &comb); if (rc != ECSIMD_HIP_OK) return rc;
  const gc_layout L = gc_plan(ctx->workspace, n);
  sm2_secret_product(ctx, rec, L, comb, d, qx, qy, n);
  launch::sm2_key_range(ctx->stream, rec.N, d, qx, qy, ok, n);
  const hipError_t err = wipe_workspace(ctx, L.bytes, hipGetLastError());                              // the Jacobian d G (and the ladder route's adjusted copy of d)
  return err == hipSuccess ? ECSIMD_HIP_OK : fail(ctx, err, "sm2_pubkey launch"); }

int ecsimd_sm2_verify_digest(ecsimd_hip_ctx* ctx, int curve, const uint64_t* e, const uint64_t* r, const uint64_t* s_, const uint64_t* qx, const uint64_t* qy, uint8_t* ok,
                             size_t n) {
  REQUIRE_CTX(); REQUIRE_PTR(e); REQUIRE_PTR(r); REQUIRE_PTR(s_); REQUIRE_PTR(qx); REQUIRE_PTR(qy);
  if (!ok && n) return bad(ctx, "ok is null");
  curve_record rec; int rc = sm2_require(ctx, curve, &rec); if (rc != ECSIMD_HIP_OK) return rc;
  if (n != 0 && any_alias({ok}, {e, r, s_, qx, qy})) return bad(ctx, "sm2_verify_digest: ok must not alias an input");
  ENTER();
  return sm2_verify_impl(ctx, curve, rec, e, nullptr, r, s_, qx, qy, ok, n); }

int ecsimd_sm2_verify(ecsimd_hip_ctx* ctx, int curve, const uint64_t* qx, const uint64_t* qy, const uint8_t* id, size_t id_bytes, size_t id_stride, const uint8_t* msg,
                      size_t msg_bytes, size_t stride_bytes, const uint32_t* lens, const uint64_t* r, const uint64_t* s_, uint8_t* ok, size_t n) {
  REQUIRE_CTX(); REQUIRE_PTR(r); REQUIRE_PTR(s_); REQUIRE_PTR(qx); REQUIRE_PTR(qy);
  if (!ok && n) return bad(ctx, "ok is null");
  curve_record rec; int rc = sm2_require(ctx, curve, &rec); if (rc != ECSIMD_HIP_OK) return rc;
  rc = sm2_id_args(ctx, id, id_bytes, id_stride, n); if (rc != ECSIMD_HIP_OK) return rc;
  rc = sm2_msg_args(ctx, msg, &msg_bytes, stride_bytes, lens, n); if (rc != ECSIMD_HIP_OK) return rc;
  if (n != 0 && any_alias({ok}, {r, s_, qx, qy, id, msg, lens})) return bad(ctx, "sm2_verify: ok must not alias an input");
  ENTER();
  const sm2_message M = {id, id_bytes, id_stride, msg, msg_bytes, stride_bytes, lens};
  return sm2_verify_impl(ctx, curve, rec, nullptr, &M, r, s_, qx, qy, ok, n); }

int ecsimd_sm2_sign_digest(ecsimd_hip_ctx* ctx, int curve, const uint64_t* e, const uint64_t* d, const uint64_t* k, uint64_t* r, uint64_t* s_, uint8_t* ok, size_t n, int flags) {
  REQUIRE_CTX(); REQUIRE_PTR(e); REQUIRE_PTR(d); REQUIRE_PTR(r); REQUIRE_PTR(s_);
  if (k && !aligned16(k)) return bad(ctx, "k is not 16-byte aligned");
  if (!ok && n) return bad(ctx, "ok is null");
  if (flags != 0) return bad(ctx, "sm2_sign_digest: flags must be 0");
  curve_record rec; int rc = sm2_require(ctx, curve, &rec); if (rc != ECSIMD_HIP_OK) return rc;
  nonce_plan P; if (!k) { rc = nonce_lookup(ctx, curve, &P); if (rc != ECSIMD_HIP_OK) return rc; }
  if (n != 0 && any_alias({r, s_, ok}, {e, d, k})) return bad(ctx, "sm2_sign_digest: r, s and ok must not alias an input or each other");
  ENTER();
  if (gc_plan(nullptr, n).chunk != n) return bad(ctx, "sm2_sign_digest: at most 2^22 signatures per call");
  rc = ensure_workspace(ctx, sm2_sign_plan(nullptr, n, k == nullptr).bytes);
  if (rc != ECSIMD_HIP_OK) return rc;
  const uint32_t* comb; rc = ensure_sm2_comb(ctx, curve, rec, &comb); if (rc != ECSIMD_HIP_OK) return rc;
  const sm2_sign_layout L = sm2_sign_plan(ctx->workspace, n, k == nullptr);
  if (!k) launch::rfc6979_nonce(ctx->stream, P.order, e, d, L.K.k, L.K.state, L.K.retry, ok, n, P.cap);              // its verdict is overwritten: a refused lane has k = 0
  const uint64_t* nonce = k ? k : L.K.k;
  sm2_secret_product(ctx, rec, L.G, comb, nonce, L.G.gx, nullptr, n);
  launch::sm2_sign_scalars(ctx->stream, rec.N, e, d, nonce, L.G.gx, r, s_, ok, n);
  const hipError_t err = wipe_workspace(ctx, L.bytes, hipGetLastError());                              // the nonce and K, V behind it, the Jacobian k G, x(k G)
  return err == hipSuccess ? ECSIMD_HIP_OK : fail(ctx, err, "sm2_sign_digest launch"); }

// ---- Multi-scalar multiplication and the point sum (include/ecsimd_msm.h; msm_stages.cuh has the stages).  PUBLIC data.  msm_schedule_of is the ONE place that turns
// (n, bits, flags) into sizes: ecsimd_msm_plan reports it, ecsimd_msm enqueues from it, tools/msm_model.py restates it.  Nothing here looks at the data.  The
// bucket route is ONE driver (bucket_sum_run) and ONE layout (msm_carve) for both curve forms: they differ in the planes of a point and in six launchers.
namespace {
int floor_log2(size_t v) { int r = 0; while (v >>= 1) ++r; return r; }
int ceil_log2(size_t v) { return v <= 1 ? 0 : floor_log2(v - 1) + 1; }
int tree_passes(size_t count) { int p = 0; while (count > 1) { count = (count + launch::MSM_TREE_FAN - 1) / launch::MSM_TREE_FAN; ++p; } return p; }
size_t round16(size_t b) { return (b + 15) / 16 * 16; }
struct msm_schedule {
  ecsimd_msm_plan_t plan;
  size_t T, K, slices, per_window, chunk_lanes, front_lanes;      // BUCKETS: entries, keys, slice lanes, chunks per window, their product with the windows; LANES: the affine tree's lanes
  size_t planes;                                                  // BUCKETS: field elements per point of the sum: 3 (Jacobian) or 4 (extended Edwards); a decoded term has one fewer
  size_t elem;                                                    // BUCKETS: bytes of a field element in the workspace: 32, or 48 on BLS12-381 (scalars are 32 on every curve)
};
// The workspace of a call, carved from `base` (nullptr: sizes only).
struct msm_blocks {
  uint32_t *counter, *hist, *start, *cursor, *sorted;   // counter (invalid points, broken invariants) and hist are ONE block, zeroed by one kernel
  uint64_t *kk, *px, *py, *buckets, *partial, *tree;    // BUCKETS: the decoded terms are planes - 1 planes of n from px on (Jacobian: px, py; Edwards: ed_precomp's three)
                                                        // LANES: kk, px, py = the sanitized scalars and points, buckets / partial = the affine products (ox, oy)
  size_t zero_bytes, reserve;                           // the length of that block; LANES: what run_varwin leaves alone at the start of the workspace
};
msm_blocks msm_carve(const msm_schedule& S, size_t n, void* base, size_t* bytes) {
  msm_blocks B = {};
  carve c = carve_from(base);
  if (S.plan.route == ECSIMD_MSM_ALG_BUCKETS) {
    B.zero_bytes = round16(16 + 4 * S.K);
    B.counter = static_cast<uint32_t*>(carve_bytes(c, B.zero_bytes)); B.hist = B.counter ? B.counter + 4 : nullptr;
    B.start = static_cast<uint32_t*>(carve_bytes(c, round16(4 * (S.K + 1))));
    B.cursor = static_cast<uint32_t*>(carve_bytes(c, round16(4 * S.K)));
    B.sorted = static_cast<uint32_t*>(carve_bytes(c, round16(4 * S.T)));
    const auto elements = [&](size_t m) { return static_cast<uint64_t*>(carve_bytes(c, m * S.elem)); };
    B.kk = carve_limbs(c, n); B.px = elements(n); B.py = elements((S.planes - 2) * n);
    B.buckets = elements(S.planes * S.K); B.partial = elements(S.planes * 2 * S.slices); B.tree = elements(S.planes * S.chunk_lanes);
  } else {
    B.zero_bytes = 32;                                  // (32: run_varwin's scratch behind `reserve` stays 32-byte aligned)
    B.counter = static_cast<uint32_t*>(carve_bytes(c, 32));
    B.kk = carve_limbs(c, n); B.px = carve_limbs(c, n); B.py = carve_limbs(c, n);
    B.buckets = carve_limbs(c, n); B.partial = carve_limbs(c, n); B.tree = carve_limbs(c, 3 * S.front_lanes);
    B.reserve = c.bytes;
    (void)carve_bytes(c, launch::varwin_scratch_bytes(chunk_of(n, VARWIN_CHUNK)));
  }
  *bytes = c.bytes;
  return B;
}
bool msm_schedule_of(size_t n, int bits, int flags, msm_schedule* S, size_t planes = 3, size_t elem = 32) {
  if (bits < 1 || bits > 256 || n > ECSIMD_MSM_MAX_N) return false;
  if (flags != ECSIMD_MSM_ALG_AUTO && flags != ECSIMD_MSM_ALG_BUCKETS && flags != ECSIMD_MSM_ALG_LANES) return false;
  *S = msm_schedule();
  S->planes = planes; S->elem = elem;
  ecsimd_msm_plan_t& P = S->plan;
  P.route = flags != ECSIMD_MSM_ALG_AUTO ? flags : n >= ECSIMD_MSM_AUTO_THRESHOLD ? ECSIMD_MSM_ALG_BUCKETS : ECSIMD_MSM_ALG_LANES;
  if (n == 0) { P.launches = 1; P.max_chain = 0; return true; }                  // the last kernel alone writes the empty sum
  const int fan = launch::MSM_TREE_FAN;
  if (P.route == ECSIMD_MSM_ALG_BUCKETS) {
    int c = floor_log2(n) - 4; if (c < 2) c = 2; if (c > 16) c = 16; if (c > bits) c = bits;
    P.windows = (bits + c - 1) / c;
    c = (bits + P.windows - 1) / P.windows;             // the same number of windows, evenly wide: no narrow top window whose few buckets hold every term
    P.c = c; P.buckets = 1u << c;
    const uint32_t L = (1u << ((ceil_log2(n) + 1) / 2)) / 4; P.L = L < 4 ? 4 : L;
    uint32_t m = 1u << ((c + 1) / 2); if (m > 32) m = 32; if (m < 2) m = 2; if (m > P.buckets) m = P.buckets; P.m = m;
    S->T = n * (size_t)P.windows; S->K = (size_t)P.windows << c; S->slices = (S->T + P.L - 1) / P.L;
    S->per_window = P.buckets / m; S->chunk_lanes = S->per_window * P.windows;
    const size_t chain[] = {P.L, (n + P.L - 1) / P.L + 1, 2 * (size_t)m + 2 * (size_t)c, (size_t)fan, (size_t)P.windows * (c + 1)};
    for (size_t v : chain) if (v > P.max_chain) P.max_chain = (uint32_t)v;
    P.launches = 8 + tree_passes(S->per_window);        // zero, digits, scan, scatter, slices, combine, chunks, the tree's passes, the last kernel
  } else {
    S->front_lanes = (n + fan - 1) / fan;
    P.max_chain = fan;
    P.launches = 4 + 5 * (int)((n + VARWIN_CHUNK - 1) / VARWIN_CHUNK) + tree_passes(S->front_lanes);   // zero, sanitize, the products (five kernels on P-256, three on secp256k1: the plan has no curve and reports the larger), the affine tree, the tree, the last kernel
  }
  (void)msm_carve(*S, n, nullptr, &P.workspace_bytes);
  return true;
}
// arr[g * stride ..]: `groups` runs of `count` elements summed into their first, fan-in 16 per launch
extern "C++" template <class ML> void tree_run(hipStream_t s, uint64_t* arr, size_t total, size_t count, size_t stride, size_t groups) {
  const int fan = launch::MSM_TREE_FAN;
  while (count > 1) {
    const size_t lanes = (count + fan - 1) / fan;
    ML::tree(s, arr, total, count, stride, groups, lanes, fan);
    count = lanes;
  }
}
// The bucket route for either curve form (the empty sum, on any route, is its last kernel alone).  A sum type names the group's launchers -- ML: combine, chunks,
// tree; its own digits, slices and finish, which carry the terms as the caller gives them and the result as the group writes it -- and `what` for the error text.
// offset: the bytes at the start of the workspace that are the caller's (the batch verifications keep their own arrays there); the blocks are carved behind them.
extern "C++" template <class Sum> int bucket_sum_run(ecsimd_hip_ctx* ctx, const msm_schedule& S, const Sum& sum, uint8_t* finite, uint32_t* invalid, size_t n, int bits, size_t offset) {
  using ML = typename Sum::ML;
  const ecsimd_msm_plan_t& P = S.plan;
  hipStream_t s = ctx->stream;
  if (n == 0) sum.finish(s, nullptr, 0, 0, 0, 0, nullptr, finite, invalid);
  else {
    const int rc = ensure_workspace(ctx, offset + P.workspace_bytes);
    if (rc != ECSIMD_HIP_OK) return rc;
    size_t bytes = 0;
    const msm_blocks B = msm_carve(S, n, reinterpret_cast<uint8_t*>(ctx->workspace) + offset, &bytes);
    launch::msm_zero(s, B.counter, B.zero_bytes);
    sum.digits(s, B, n, bits, P.c, P.windows);
    launch::msm_scan(s, B.hist, B.start, B.cursor, S.K);
    launch::msm_scatter(s, B.kk, B.cursor, B.sorted, B.counter + 1, n, S.T, P.c, P.windows);
    sum.slices(s, B, n, S.T, P.L, S.slices, P.c, S.K);
    ML::combine(s, B.start, B.buckets, B.partial, B.counter + 1, P.L, S.slices, P.c, S.K);
    ML::chunks(s, B.buckets, B.tree, S.chunk_lanes, S.per_window, P.c, (int)P.m, S.K);
    tree_run<ML>(s, B.tree, S.chunk_lanes, S.per_window, S.per_window, (size_t)P.windows);
    sum.finish(s, B.tree, S.chunk_lanes, S.per_window, P.windows, P.c, B.counter, finite, invalid);
  }
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? ECSIMD_HIP_OK : fail(ctx, e, Sum::what);
}
extern "C++" template <int CV> struct jacobian_sum {
  using ML = launch::msm_launch<CV>;
  static constexpr const char* what = "msm launch";
  const uint64_t *k, *x, *y; uint64_t *rx, *ry;
  void digits(hipStream_t s, const msm_blocks& B, size_t n, int bits, int c, int windows) const { ML::digits(s, k, x, y, B.kk, B.px, B.py, B.hist, B.counter, n, bits, c, windows); }
  void slices(hipStream_t s, const msm_blocks& B, size_t n, size_t T, size_t L, size_t slices, int c, size_t K) const {
    ML::slices(s, B.sorted, B.kk, B.px, B.py, B.start, B.buckets, B.partial, B.counter + 1, n, T, L, slices, c, K);
  }
  void finish(hipStream_t s, const uint64_t* arr, size_t total, size_t stride, int windows, int c, const uint32_t* counter, uint8_t* finite, uint32_t* invalid) const {
    ML::finish(s, arr, total, stride, windows, c, counter, rx, ry, finite, invalid);
  }
};
extern "C++" template <int CV> int msm_run(ecsimd_hip_ctx* ctx, const msm_schedule& S, const uint64_t* k, const uint64_t* x, const uint64_t* y, uint64_t* rx, uint64_t* ry, uint8_t* finite,
                              uint32_t* invalid, size_t n, int bits, size_t offset = 0) {
  using ML = launch::msm_launch<CV>;
  if (n == 0 || S.plan.route == ECSIMD_MSM_ALG_BUCKETS) return bucket_sum_run(ctx, S, jacobian_sum<CV>{k, x, y, rx, ry}, finite, invalid, n, bits, offset);
  hipStream_t s = ctx->stream;
  int rc = ensure_workspace(ctx, offset + S.plan.workspace_bytes);
  if (rc != ECSIMD_HIP_OK) return rc;
  size_t bytes = 0;
  const msm_blocks B = msm_carve(S, n, reinterpret_cast<uint8_t*>(ctx->workspace) + offset, &bytes);
  launch::msm_zero(s, B.counter, B.zero_bytes);
  ML::sanitize(s, k, x, y, B.kk, B.px, B.py, B.counter, n, bits);
  rc = run_varwin(ctx, CV, B.kk, 4, B.px, B.py, B.buckets, B.partial, n, ECSIMD_HIP_OUT_AFFINE | ECSIMD_HIP_ALG_WINDOWED, offset + B.reserve);   // the workspace is large enough: nothing moves
  if (rc != ECSIMD_HIP_OK) return rc;
  ML::tree_affine(s, B.buckets, B.partial, false, B.counter, B.tree, n, S.front_lanes, launch::MSM_TREE_FAN);
  tree_run<ML>(s, B.tree, S.front_lanes, S.front_lanes, 0, 1);
  ML::finish(s, B.tree, S.front_lanes, 0, 1, 0, B.counter, rx, ry, finite, invalid);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? ECSIMD_HIP_OK : fail(ctx, e, "msm launch");
}
extern "C++" template <int CV> int point_sum_run(ecsimd_hip_ctx* ctx, const uint64_t* x, const uint64_t* y, uint64_t* rx, uint64_t* ry, uint8_t* finite, uint32_t* invalid, size_t n) {
  using ML = launch::msm_launch<CV>;
  hipStream_t s = ctx->stream;
  const int fan = launch::MSM_TREE_FAN;
  if (n == 0) { ML::finish(s, nullptr, 0, 0, 0, 0, nullptr, rx, ry, finite, invalid); const hipError_t e0 = hipGetLastError(); return e0 == hipSuccess ? ECSIMD_HIP_OK : fail(ctx, e0, "msm launch"); }
  const size_t front = (n + fan - 1) / fan;
  carve c = carve_from(nullptr); (void)carve_bytes(c, 16); (void)carve_limbs(c, 3 * front);
  int rc = ensure_workspace(ctx, c.bytes);
  if (rc != ECSIMD_HIP_OK) return rc;
  c = carve_from(ctx->workspace);
  uint32_t* counter = static_cast<uint32_t*>(carve_bytes(c, 16)); uint64_t* tree = carve_limbs(c, 3 * front);
  launch::msm_zero(s, counter, 16);
  ML::tree_affine(s, x, y, true, counter, tree, n, front, fan);
  tree_run<ML>(s, tree, front, front, 0, 1);
  ML::finish(s, tree, front, 0, 1, 0, counter, rx, ry, finite, invalid);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? ECSIMD_HIP_OK : fail(ctx, e, "point_sum launch");
}
int msm_check_common(ecsimd_hip_ctx* ctx, int curve, const uint64_t* x, const uint64_t* y, uint64_t* rx, uint64_t* ry, uint8_t* finite, uint32_t* invalid, size_t n) {
  if (curve >= ECSIMD_HIP_FIRST_REGISTERED_CURVE) return bad(ctx, "registered curves have no multi-scalar multiplication: ECSIMD_HIP_P256 and ECSIMD_HIP_SECP256K1 only");
  REQUIRE_CURVE();
  REQUIRE_PTR(x); REQUIRE_PTR(y);
  if (!rx || !ry || !finite) return bad(ctx, "msm: rx, ry or finite is null");
  if (!aligned16(rx) || !aligned16(ry)) return bad(ctx, "msm: rx or ry is not 16-byte aligned");
  if (invalid && (reinterpret_cast<uintptr_t>(invalid) & 3u)) return bad(ctx, "msm: invalid is not 4-byte aligned");
  if (invalid ? any_alias({rx, ry, finite, invalid}, {x, y}) : any_alias({rx, ry, finite}, {x, y})) return bad(ctx, "msm: an output must not alias an input or another output");
  return ECSIMD_HIP_OK;
}
}  // namespace

int ecsimd_msm_plan(size_t n, int bits, int flags, ecsimd_msm_plan_t* out) {
  msm_schedule S;
  if (!out || !msm_schedule_of(n, bits, flags, &S)) return ECSIMD_HIP_ERR_BAD_ARG;
  *out = S.plan;
  return ECSIMD_HIP_OK; }

int ecsimd_msm(ecsimd_hip_ctx* ctx, int curve, const uint64_t* k, const uint64_t* x, const uint64_t* y, uint64_t* rx, uint64_t* ry, uint8_t* finite, uint32_t* invalid,
               size_t n, int bits, int flags) {
  REQUIRE_CTX();
  int rc = msm_check_common(ctx, curve, x, y, rx, ry, finite, invalid, n);
  if (rc != ECSIMD_HIP_OK) return rc;
  REQUIRE_PTR(k);
  if (n && (overlaps(k, rx) || overlaps(k, ry) || overlaps(k, finite) || overlaps(k, invalid))) return bad(ctx, "msm: an output must not alias an input or another output");
  if (bits < 1 || bits > 256) return bad(ctx, "msm: bits must be 1 .. 256");
  if (n > ECSIMD_MSM_MAX_N) return bad(ctx, "msm: n is above ECSIMD_MSM_MAX_N: chain chunks through ecsimd_msm_point_sum");
  msm_schedule S;
  if (!msm_schedule_of(n, bits, flags, &S)) return bad(ctx, "msm: flags must be ECSIMD_MSM_ALG_AUTO, ECSIMD_MSM_ALG_BUCKETS or ECSIMD_MSM_ALG_LANES");
  const hipError_t e0 = hipSetDevice(ctx->device); if (e0 != hipSuccess) return fail(ctx, e0, "hipSetDevice");
  return curve == ECSIMD_HIP_P256 ? msm_run<CURVE_P256>(ctx, S, k, x, y, rx, ry, finite, invalid, n, bits) : msm_run<CURVE_SECP256K1>(ctx, S, k, x, y, rx, ry, finite, invalid, n, bits); }

int ecsimd_msm_point_sum(ecsimd_hip_ctx* ctx, int curve, const uint64_t* x, const uint64_t* y, uint64_t* rx, uint64_t* ry, uint8_t* finite, uint32_t* invalid, size_t n) {
  REQUIRE_CTX();
  int rc = msm_check_common(ctx, curve, x, y, rx, ry, finite, invalid, n);
  if (rc != ECSIMD_HIP_OK) return rc;
  if ((n + launch::MSM_TREE_FAN - 1) / launch::MSM_TREE_FAN > MAX_LAUNCH) return bad(ctx, "batch too large");
  const hipError_t e0 = hipSetDevice(ctx->device); if (e0 != hipSuccess) return fail(ctx, e0, "hipSetDevice");
  return curve == ECSIMD_HIP_P256 ? point_sum_run<CURVE_P256>(ctx, x, y, rx, ry, finite, invalid, n) : point_sum_run<CURVE_SECP256K1>(ctx, x, y, rx, ry, finite, invalid, n); }

// ---- BIP-340 batch verification (include/ecsimd_schnorr_batch.h; k_schnorr_batch.hip has the stages, tools/schnorr_batch_model.py the definition).  PUBLIC data.
// sb_schedule_of is the ONE place that turns (n, msg_bytes, flags) into sizes: ecsimd_schnorr_batch_plan reports it, the calls enqueue from it.  The MSM route's
// workspace: the call's own arrays first (sb_carve), then the blocks of the two bucket sums, which run one after the other and share their bytes.
// What this call and Ed25519 batch verification do alike -- the fan-16 trees, the workspace of the MSM route, the shared checks -- is the batch_* functions' here.
namespace {
size_t fan_lanes(size_t count) { return (count + launch::BATCH_FAN - 1) / launch::BATCH_FAN; }
int fan_passes(size_t count) { int p = 0; while (count > 1) { count = fan_lanes(count); ++p; } return p; }
size_t fan_elements(size_t count) { size_t t = 0; while (count > 1) { count = fan_lanes(count); t += count; } return t; }      // every level below the leaves
// The MSM route of a batch of n >= 1 signatures: a sum of n terms with 128-bit scalars, then one of n + 1 terms with key_bits-bit scalars.
struct batch_sums { msm_schedule r, key; };
bool batch_sums_of(size_t n, int key_bits, size_t planes, batch_sums* S) {
  return msm_schedule_of(n, 128, ECSIMD_MSM_ALG_BUCKETS, &S->r, planes) && msm_schedule_of(n + 1, key_bits, ECSIMD_MSM_ALG_BUCKETS, &S->key, planes);
}
// ... its bytes for exactly n: the call's own arrays, then the larger of the two sums' blocks (they run one after the other)
size_t batch_msm_bytes(size_t own, size_t n, int key_bits, size_t planes) {
  batch_sums S;
  if (!batch_sums_of(n, key_bits, planes, &S)) return 0;
  return own + (S.r.plan.workspace_bytes > S.key.plan.workspace_bytes ? S.r.plan.workspace_bytes : S.key.plan.workspace_bytes);
}
// What a batch of n needs, and what every smaller batch would: the bucket sums' blocks are not monotone in the number of terms (a wider window means fewer
// sorted entries), but between powers of two they are -- the window width, the bucket count and the segment split are fixed there and only the entries
// grow --, so the largest need below n is met at n itself or next to a power of two.  A context warmed up at n then serves every smaller batch in a capture.
size_t batch_workspace_bytes(size_t n, size_t (*bytes_for_exactly)(size_t)) {
  size_t need = bytes_for_exactly(n);
  for (size_t p = 2; p <= n + 2; p <<= 1)
    for (size_t m = p - 2; m <= p && m <= n; ++m)
      if (m >= 1 && bytes_for_exactly(m) > need) need = bytes_for_exactly(m);
  return need;
}
// ... and its kernels: zero, front, seed, scalars, accept; the two trees; the two sums
int batch_msm_launches(size_t n, const batch_sums& S) {
  const int levels = fan_passes(n);
  return 5 + levels + (levels > 1 ? levels : 1) + S.r.plan.launches + S.key.plan.launches;
}
// Enqueues the hash tree over the n leaves, a level per launch, the levels one behind the other in `nodes`; returns the root's level (n = 1: the leaf).
const uint64_t* batch_hash_tree(hipStream_t s, void (*node)(hipStream_t, const uint64_t*, size_t, uint64_t*), const uint64_t* leaf, uint64_t* nodes, size_t n) {
  const uint64_t* level = leaf;
  for (size_t count = n; count > 1;) {
    node(s, level, count, nodes);
    count = fan_lanes(count); level = nodes; nodes += 4 * count;
  }
  return level;
}
// Enqueues the tree of additions over the n scalars at `in`, the levels one behind the other in `levels`: sum(in, count, out, last); the last level (one lane,
// even for n = 1) writes to last_out, where it is term n of the key sum.
extern "C++" template <class Sum> void batch_scalar_sum(const uint64_t* in, uint64_t* levels, uint64_t* last_out, size_t n, Sum sum) {
  for (size_t count = n, lanes = 0; lanes != 1; count = lanes) {
    lanes = fan_lanes(count);
    const bool last = lanes == 1;
    sum(in, count, last ? last_out : levels, last);
    in = levels; levels += 4 * lanes;
  }
}
// Two byte ranges that share a byte (an empty or a null one shares none).
struct byte_range { const void* p; size_t bytes; };
bool ranges_overlap(const void* a, size_t abytes, const void* b, size_t bbytes) {
  if (!a || !b || !abytes || !bbytes) return false;
  const uintptr_t pa = reinterpret_cast<uintptr_t>(a), pb = reinterpret_cast<uintptr_t>(b);
  return pa < pb + bbytes && pb < pa + abytes;
}
// What the batch calls check alike: the cap on n, the messages by the call's own rule, and that `out` (what the call writes) overlaps no input.
extern "C++" template <class Messages> int batch_check(ecsimd_hip_ctx* ctx, const char* what, size_t n, Messages messages, byte_range out, std::initializer_list<byte_range> in) {
  char text[128];
  snprintf(text, sizeof text, "%s: n is above ECSIMD_MSM_MAX_N - 1: verify chunks and AND their verdicts", what);
  if (n > ECSIMD_MSM_MAX_N - 1) return bad(ctx, text);
  const int rc = messages(); if (rc != ECSIMD_HIP_OK) return rc;
  snprintf(text, sizeof text, "%s: the output must not overlap an input", what);
  for (const byte_range& r : in) if (ranges_overlap(out.p, out.bytes, r.p, r.bytes)) return bad(ctx, text);
  return ECSIMD_HIP_OK;
}
struct sb_blocks {
  launch::schnorr_batch_head* head;
  uint64_t *E, *leaf, *nodes, *a, *ae, *as, *sums, *Px, *Py, *Rx, *Ry;      // ae, Px, Py: n + 1 elements, the last one the G term; nodes, sums: the trees' levels, one behind the other
  uint8_t* valid;
};
sb_blocks sb_carve(size_t n, void* base, size_t* bytes) {
  sb_blocks B; carve c = carve_from(base);
  B.head = static_cast<launch::schnorr_batch_head*>(carve_bytes(c, sizeof(launch::schnorr_batch_head)));
  B.E = carve_limbs(c, n); B.leaf = carve_limbs(c, n); B.nodes = carve_limbs(c, fan_elements(n));
  B.a = carve_limbs(c, n); B.ae = carve_limbs(c, n + 1); B.as = carve_limbs(c, n); B.sums = carve_limbs(c, fan_elements(n));
  B.Px = carve_limbs(c, n + 1); B.Py = carve_limbs(c, n + 1); B.Rx = carve_limbs(c, n); B.Ry = carve_limbs(c, n);
  B.valid = carve_flags(c, n);
  (void)carve_bytes(c, (32 - c.bytes % 32) % 32);      // the sums' blocks start on 32 bytes
  *bytes = c.bytes;
  return B;
}
struct sb_schedule { ecsimd_schnorr_batch_plan_t plan; batch_sums sums; };
size_t sb_msm_bytes(size_t n) { size_t own = 0; (void)sb_carve(n, nullptr, &own); return batch_msm_bytes(own, n, 256, 3); }
bool sb_route_ok(int flags) { return flags == ECSIMD_SCHNORR_BATCH_AUTO || flags == ECSIMD_SCHNORR_BATCH_MSM || flags == ECSIMD_SCHNORR_BATCH_LANES; }
bool sb_schedule_of(size_t n, size_t msg_bytes, int flags, sb_schedule* S) {
  if (n > ECSIMD_MSM_MAX_N - 1 || msg_bytes > ((size_t)1 << 40) || !sb_route_ok(flags)) return false;
  *S = sb_schedule();
  ecsimd_schnorr_batch_plan_t& P = S->plan;
  P.route = flags != ECSIMD_SCHNORR_BATCH_AUTO ? flags : n >= ECSIMD_SCHNORR_BATCH_AUTO_THRESHOLD ? ECSIMD_SCHNORR_BATCH_MSM : ECSIMD_SCHNORR_BATCH_LANES;
  if (n == 0) { P.launches = 1; return true; }                                   // the reduction kernel alone writes the empty batch's verdict
  if (P.route == ECSIMD_SCHNORR_BATCH_MSM) {
    if (!batch_sums_of(n, 256, 3, &S->sums)) return false;
    P.workspace_bytes = batch_workspace_bytes(n, sb_msm_bytes);
    P.launches = batch_msm_launches(n, S->sums);
  } else {
    P.workspace_bytes = schnorr_verify_bytes(n, true);
    P.launches = 1 + 9 * (int)((n + VARWIN_CHUNK - 1) / VARWIN_CHUNK);
  }
  return true;
}
// What the two calls check alike, `out` being the `out_bytes` bytes either writes; fills O.
int sb_check(ecsimd_hip_ctx* ctx, const char* what, const uint64_t* px, const uint8_t* msg, size_t msg_bytes, size_t stride_bytes, const uint64_t* r, const uint64_t* s_,
             const void* out, size_t out_bytes, size_t n, group_order* O) {
  REQUIRE_PTR(px); REQUIRE_PTR(r); REQUIRE_PTR(s_);
  const size_t msg_extent = n ? (n - 1) * stride_bytes + msg_bytes : 0;
  return batch_check(ctx, "schnorr batch", n, [&] { return schnorr_common(ctx, what, msg, msg_bytes, stride_bytes, n, O); }, {out, out_bytes},
                     {{px, 32 * n}, {r, 32 * n}, {s_, 32 * n}, {msg, msg_extent}});
}
// Stages 1 to 3 for n >= 1: the front, the hash tree, the seed, the scalars.  `a`: where the randomizers go (B.a, or the caller's array).
void sb_randomizers(ecsimd_hip_ctx* ctx, const group_order& O, const sb_blocks& B, const uint64_t* px, const uint8_t* msg, size_t msg_bytes, size_t stride_bytes,
                    const uint64_t* r, const uint64_t* s_, uint64_t* a, size_t n) {
  hipStream_t s = ctx->stream;
  launch::msm_zero(s, B.head, sizeof(launch::schnorr_batch_head));
  launch::schnorr_batch_front(s, O.words, px, r, s_, msg, msg_bytes, stride_bytes, B.E, B.leaf, B.Px, B.Py, B.Rx, B.Ry, B.valid, B.head, n);
  launch::schnorr_batch_seed(s, batch_hash_tree(s, launch::schnorr_batch_node, B.leaf, B.nodes, n), n, B.head);
  launch::schnorr_batch_scalars(s, O.N, B.head, B.E, s_, B.valid, a, B.ae, B.as, n);
}
}  // namespace

int ecsimd_schnorr_batch_plan(size_t n, size_t msg_bytes, int flags, ecsimd_schnorr_batch_plan_t* out) {
  sb_schedule S;
  if (!out || !sb_schedule_of(n, msg_bytes, flags, &S)) return ECSIMD_HIP_ERR_BAD_ARG;
  *out = S.plan;
  return ECSIMD_HIP_OK; }

int ecsimd_schnorr_verify_batch(ecsimd_hip_ctx* ctx, const uint64_t* px, const uint8_t* msg, size_t msg_bytes, size_t stride_bytes,
                                const uint64_t* r, const uint64_t* s_, uint8_t* ok, size_t n, int flags) {
  REQUIRE_CTX();
  if (!ok) return bad(ctx, "schnorr_verify_batch: ok is null");
  if (!sb_route_ok(flags)) return bad(ctx, "schnorr_verify_batch: flags must be ECSIMD_SCHNORR_BATCH_AUTO, ECSIMD_SCHNORR_BATCH_MSM or ECSIMD_SCHNORR_BATCH_LANES");
  group_order O;
  int rc = sb_check(ctx, "schnorr_verify_batch", px, msg, msg_bytes, stride_bytes, r, s_, ok, 1, n, &O); if (rc != ECSIMD_HIP_OK) return rc;
  sb_schedule S;
  if (!sb_schedule_of(n, msg_bytes, flags, &S)) return bad(ctx, "schnorr_verify_batch: no schedule for these arguments");
  const hipError_t e0 = hipSetDevice(ctx->device); if (e0 != hipSuccess) return fail(ctx, e0, "hipSetDevice");
  hipStream_t s = ctx->stream;
  if (n == 0) launch::flags_all(s, nullptr, 0, ok);
  else if (S.plan.route == ECSIMD_SCHNORR_BATCH_LANES) {
    uint8_t* verdicts = nullptr;
    rc = schnorr_verify_run(ctx, O, px, msg, msg_bytes, stride_bytes, r, s_, nullptr, n, &verdicts); if (rc != ECSIMD_HIP_OK) return rc;
    launch::flags_all(s, verdicts, n, ok);
  } else {
    rc = ensure_workspace(ctx, S.plan.workspace_bytes); if (rc != ECSIMD_HIP_OK) return rc;      // all of it now: the sums below find it large enough, nothing moves
    size_t own = 0;
    const sb_blocks B = sb_carve(n, ctx->workspace, &own);
    sb_randomizers(ctx, O, B, px, msg, msg_bytes, stride_bytes, r, s_, B.a, n);
    batch_scalar_sum(B.as, B.sums, B.ae + 4 * n, n, [&](const uint64_t* in, size_t count, uint64_t* out, bool last) {        // sum a s, and G beside it
      launch::schnorr_batch_sum(s, O.N, in, count, out, last ? B.Px + 4 * n : nullptr, last ? B.Py + 4 * n : nullptr);
    });
    rc = msm_run<CURVE_SECP256K1>(ctx, S.sums.r, B.a, B.Rx, B.Ry, B.head->rx[0], B.head->ry[0], &B.head->finite[0], &B.head->invalid[0], n, 128, own);
    if (rc == ECSIMD_HIP_OK) rc = msm_run<CURVE_SECP256K1>(ctx, S.sums.key, B.ae, B.Px, B.Py, B.head->rx[1], B.head->ry[1], &B.head->finite[1], &B.head->invalid[1], n + 1, 256, own);
    if (rc != ECSIMD_HIP_OK) return rc;
    launch::schnorr_batch_accept(s, B.head, ok);
  }
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? ECSIMD_HIP_OK : fail(ctx, e, "schnorr_verify_batch launch"); }

int ecsimd_schnorr_batch_randomizers(ecsimd_hip_ctx* ctx, const uint64_t* px, const uint8_t* msg, size_t msg_bytes, size_t stride_bytes,
                                     const uint64_t* r, const uint64_t* s_, uint64_t* a, size_t n) {
  REQUIRE_CTX(); REQUIRE_PTR(a);
  group_order O;
  int rc = sb_check(ctx, "schnorr_batch_randomizers", px, msg, msg_bytes, stride_bytes, r, s_, a, 32 * n, n, &O); if (rc != ECSIMD_HIP_OK) return rc;
  ENTER_ANY_SIZE();
  size_t own = 0;
  (void)sb_carve(n, nullptr, &own);
  rc = ensure_workspace(ctx, own); if (rc != ECSIMD_HIP_OK) return rc;
  sb_randomizers(ctx, O, sb_carve(n, ctx->workspace, &own), px, msg, msg_bytes, stride_bytes, r, s_, a, n);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? ECSIMD_HIP_OK : fail(ctx, e, "schnorr_batch_randomizers launch"); }

// ---- The bucket method on the Edwards curve and Ed25519 batch verification (include/ecsimd_ed25519_batch.h; k_msm_ed25519.hip has the stages,
// tools/ed25519_batch_model.py the definition).  PUBLIC data.  The sum's schedule is msm_schedule_of's BUCKETS route with four planes a point, its driver
// bucket_sum_run.  edb_schedule_of is the ONE place that turns (n, msg_bytes, flags) into the batch's sizes.
namespace {
bool edm_schedule_of(size_t n, int bits, int flags, msm_schedule* S) {
  if (flags != ECSIMD_MSM_ALG_AUTO && flags != ECSIMD_MSM_ALG_BUCKETS) return false;                 // the bucket route only
  return msm_schedule_of(n, bits, ECSIMD_MSM_ALG_BUCKETS, S, 4);
}
// out: the encoding (raw == nullptr) or raw: the extended point.
struct edwards_sum {
  using ML = launch::ed25519_msm_launch;
  static constexpr const char* what = "ed25519_msm launch";
  const uint8_t *k, *pts; uint8_t* out; uint64_t* raw;
  void digits(hipStream_t s, const msm_blocks& B, size_t n, int bits, int c, int windows) const { ML::digits(s, k, pts, B.kk, B.px, B.hist, B.counter, n, bits, c, windows); }
  void slices(hipStream_t s, const msm_blocks& B, size_t n, size_t T, size_t L, size_t slices, int c, size_t K) const {
    ML::slices(s, B.sorted, B.kk, B.px, B.start, B.buckets, B.partial, B.counter + 1, n, T, L, slices, c, K);
  }
  void finish(hipStream_t s, const uint64_t* arr, size_t total, size_t stride, int windows, int c, const uint32_t* counter, uint8_t* finite, uint32_t* invalid) const {
    ML::finish(s, arr, total, stride, windows, c, counter, out, raw, finite, invalid);
  }
};

// The per-lane cofactored rule, a chunk at a time: s, h, R's (x, y), the table of -A, valid.
struct edc_layout { uint64_t *s, *h, *rxy; void* table; uint8_t* valid; size_t bytes; };
edc_layout edc_plan(void* base, size_t chunk) {
  edc_layout L; carve c = carve_from(base);
  L.s = carve_limbs(c, chunk); L.h = carve_limbs(c, chunk); L.rxy = carve_limbs(c, 2 * chunk); L.table = carve_bytes(c, launch::ed25519_table_bytes(chunk)); L.valid = carve_flags(c, chunk);
  L.bytes = c.bytes;
  return L;
}
size_t round32(size_t b) { return (b + 31) / 32 * 32; }
size_t edc_bytes(size_t n, bool own_verdicts) { return (own_verdicts ? round32(flag_bytes(n)) : 0) + edc_plan(nullptr, chunk_of(n, ED25519_VERIFY_CHUNK)).bytes; }
// ok == nullptr: the verdicts go to the first bytes of the workspace (*verdicts), the chunk's arrays behind them.  n >= 1.
int edc_run(ecsimd_hip_ctx* ctx, const uint8_t* pk, const uint8_t* msg, size_t msg_bytes, size_t stride_bytes, const uint32_t* lens, const uint8_t* sig, uint8_t* ok, size_t n,
            bool reject_small, uint8_t** verdicts) {
  const size_t own = ok ? 0 : round32(flag_bytes(n)), chunk = chunk_of(n, ED25519_VERIFY_CHUNK);
  const int rc = ensure_workspace(ctx, edc_bytes(n, !ok));
  if (rc != ECSIMD_HIP_OK) return rc;
  uint8_t* base = reinterpret_cast<uint8_t*>(ctx->workspace);
  if (!ok) ok = base;
  if (verdicts) *verdicts = ok;
  const edc_layout L = edc_plan(base + own, chunk);
  FOR_CHUNKS(first, m, n, chunk) {
    launch::ed25519_cofactored_front(ctx->stream, *ed25519_order(), pk + 32 * first, sig + 64 * first, msg ? msg + first * stride_bytes : nullptr, msg_bytes, stride_bytes,
                                     lens ? lens + first : nullptr, reject_small, L.s, L.h, L.rxy, L.table, L.valid, m);
    launch::ed25519_cofactored_loop(ctx->stream, L.s, L.h, L.rxy, L.table, L.valid, ok + first, m);
  }
  return ECSIMD_HIP_OK;
}

struct edb_blocks {
  launch::ed25519_batch_head* head;
  uint64_t *h, *leaf, *nodes, *z, *zh, *zs, *sums, *Aenc, *Renc;      // zh, Aenc: n + 1 elements, the last one the B term; nodes, sums: the trees' levels, one behind the other
  uint8_t* valid;
};
edb_blocks edb_carve(size_t n, void* base, size_t* bytes) {
  edb_blocks B; carve c = carve_from(base);
  B.head = static_cast<launch::ed25519_batch_head*>(carve_bytes(c, sizeof(launch::ed25519_batch_head)));
  B.h = carve_limbs(c, n); B.leaf = carve_limbs(c, n); B.nodes = carve_limbs(c, fan_elements(n));
  B.z = carve_limbs(c, n); B.zh = carve_limbs(c, n + 1); B.zs = carve_limbs(c, n); B.sums = carve_limbs(c, fan_elements(n));
  B.Aenc = carve_limbs(c, n + 1); B.Renc = carve_limbs(c, n);
  B.valid = carve_flags(c, n);
  (void)carve_bytes(c, (32 - c.bytes % 32) % 32);      // the sums' blocks start on 32 bytes
  *bytes = c.bytes;
  return B;
}
constexpr int EDB_KEY_BITS = 253;                       // z h mod L and L - sum z s are below L < 2^253
struct edb_schedule { ecsimd_ed25519_batch_plan_t plan; batch_sums sums; bool reject_small; };
size_t edb_msm_bytes(size_t n) { size_t own = 0; (void)edb_carve(n, nullptr, &own); return batch_msm_bytes(own, n, EDB_KEY_BITS, 4); }
bool edb_flags_ok(int flags) {
  const int route = flags & ~ECSIMD_ED25519_REJECT_SMALL_ORDER;
  return flags >= 0 && (route == ECSIMD_ED25519_BATCH_AUTO || route == ECSIMD_ED25519_BATCH_MSM || route == ECSIMD_ED25519_BATCH_LANES);
}
bool edb_schedule_of(size_t n, size_t msg_bytes, int flags, edb_schedule* S) {
  if (n > ECSIMD_MSM_MAX_N - 1 || msg_bytes > ((size_t)1 << 40) || !edb_flags_ok(flags)) return false;
  *S = edb_schedule();
  ecsimd_ed25519_batch_plan_t& P = S->plan;
  const int route = flags & ~ECSIMD_ED25519_REJECT_SMALL_ORDER;
  S->reject_small = (flags & ECSIMD_ED25519_REJECT_SMALL_ORDER) != 0;
  P.route = route != ECSIMD_ED25519_BATCH_AUTO ? route : n >= ECSIMD_ED25519_BATCH_AUTO_THRESHOLD ? ECSIMD_ED25519_BATCH_MSM : ECSIMD_ED25519_BATCH_LANES;
  if (n == 0) { P.launches = 1; return true; }                                   // the reduction kernel alone writes the empty batch's verdict
  if (P.route == ECSIMD_ED25519_BATCH_MSM) {
    if (!batch_sums_of(n, EDB_KEY_BITS, 4, &S->sums)) return false;
    P.workspace_bytes = batch_workspace_bytes(n, edb_msm_bytes);
    P.launches = batch_msm_launches(n, S->sums);
  } else {
    P.workspace_bytes = edc_bytes(n, true);
    P.launches = 1 + 2 * (int)((n + ED25519_VERIFY_CHUNK - 1) / ED25519_VERIFY_CHUNK);
  }
  return true;
}
// What the batch calls check alike, `out` being the `out_bytes` bytes either writes; msg_bytes comes back as 0 where lens rules.
int edb_check(ecsimd_hip_ctx* ctx, const uint8_t* pk, const uint8_t* msg, size_t* msg_bytes, size_t stride_bytes, const uint32_t* lens, const uint8_t* sig, const void* out,
              size_t out_bytes, size_t n) {
  if ((!pk || !sig) && n) return bad(ctx, "ed25519 batch: pk or sig is null");
  const size_t msg_extent = n ? (n - 1) * stride_bytes + (lens ? stride_bytes : *msg_bytes) : 0;
  return batch_check(ctx, "ed25519 batch", n, [&] { return ed25519_messages(ctx, msg, msg_bytes, stride_bytes, lens, n); }, {out, out_bytes},
                     {{pk, 32 * n}, {sig, 64 * n}, {msg, msg_extent}, {lens, 4 * n}});
}
// The front, the hash tree, the seed, the scalars for n >= 1.  z: where the randomizers go; products: also z h and z s (B.zh, B.zs).
void edb_randomizers(ecsimd_hip_ctx* ctx, const edb_blocks& B, const uint8_t* pk, const uint8_t* msg, size_t msg_bytes, size_t stride_bytes, const uint32_t* lens,
                     const uint8_t* sig, bool reject_small, uint64_t* z, bool products, size_t n) {
  hipStream_t s = ctx->stream;
  launch::msm_zero(s, B.head, sizeof(launch::ed25519_batch_head));
  launch::ed25519_batch_front(s, *ed25519_order(), pk, sig, msg, msg_bytes, stride_bytes, lens, reject_small, B.h, B.leaf, B.Aenc, B.Renc, B.valid, B.head, n);
  launch::ed25519_batch_seed(s, batch_hash_tree(s, launch::ed25519_batch_node, B.leaf, B.nodes, n), n, B.head);
  launch::ed25519_batch_scalars(s, *ed25519_order(), B.head, B.h, sig, B.valid, z, products ? B.zh : nullptr, products ? B.zs : nullptr, n);
}
}  // namespace

int ecsimd_ed25519_msm_plan(size_t n, int bits, int flags, ecsimd_msm_plan_t* out) {
  msm_schedule S;
  if (!out || !edm_schedule_of(n, bits, flags, &S)) return ECSIMD_HIP_ERR_BAD_ARG;
  *out = S.plan;
  return ECSIMD_HIP_OK; }

int ecsimd_ed25519_msm(ecsimd_hip_ctx* ctx, const uint8_t* k, const uint8_t* pts, uint8_t* out, uint8_t* finite, uint32_t* invalid, size_t n, int bits, int flags) {
  REQUIRE_CTX();
  if ((!k || !pts) && n) return bad(ctx, "ed25519_msm: k or pts is null");
  if (!out || !finite) return bad(ctx, "ed25519_msm: out or finite is null");
  if (invalid && (reinterpret_cast<uintptr_t>(invalid) & 3u)) return bad(ctx, "ed25519_msm: invalid is not 4-byte aligned");
  if (bits < 1 || bits > 256) return bad(ctx, "ed25519_msm: bits must be 1 .. 256");
  if (n > ECSIMD_MSM_MAX_N) return bad(ctx, "ed25519_msm: n is above ECSIMD_MSM_MAX_N");
  msm_schedule S;
  if (!edm_schedule_of(n, bits, flags, &S)) return bad(ctx, "ed25519_msm: flags must be 0 or ECSIMD_MSM_ALG_BUCKETS: the bucket route only");
  const void* outs[3] = {out, finite, invalid}; const size_t out_bytes[3] = {32, 1, 4};
  for (int a = 0; a < 3; ++a) {
    if (ranges_overlap(outs[a], out_bytes[a], k, 32 * n) || ranges_overlap(outs[a], out_bytes[a], pts, 32 * n)) return bad(ctx, "ed25519_msm: an output must not overlap an input or another output");
    for (int b = a + 1; b < 3; ++b) if (ranges_overlap(outs[a], out_bytes[a], outs[b], out_bytes[b])) return bad(ctx, "ed25519_msm: an output must not overlap an input or another output");
  }
  const hipError_t e0 = hipSetDevice(ctx->device); if (e0 != hipSuccess) return fail(ctx, e0, "hipSetDevice");
  return bucket_sum_run(ctx, S, edwards_sum{k, pts, out, nullptr}, finite, invalid, n, bits, 0); }

// ---- BLS12-381 G1 and G2 (include/ecsimd_bls12_381.h, include/ecsimd_bls12_381_g2.h; k_bls12_381.inc as k_bls12_381.hip and k_bls12_381_g2.hip;
// tools/bls12_381_model.py and tools/bls12_381_g2_model.py the definitions).  PUBLIC data.  ONE host layer over what a group's sizes are: bls381_g1 and bls381_g2
// below.  A field element is ELEM bytes in the workspace and compressed, a point 2 ELEM bytes uncompressed.  The bucket route is msm_schedule_of's with ELEM-byte
// field elements and bucket_sum_run; bls381_schedule_of is the ONE place that turns (n, bits, flags) into a group's sizes, the LANES route included (its products
// need no per-lane table, so its workspace is the counter and one Jacobian array).  The messages spell the widths out: "in48, out96" for G1, "in96, out192" for G2.
extern "C++" {
namespace {
struct bls381_g1 {
  using ML = launch::bls381_launch<g1_curve>;
  static constexpr size_t ELEM = 48, AUTO_THRESHOLD = ECSIMD_BLS12_381_MSM_AUTO_THRESHOLD;
  static constexpr const char *name = "bls12_381_g1", *raw_name = "bls12_381_raw", *flag_stem = "ECSIMD_BLS12_381", *msm_launch = "bls12_381_g1_msm launch";
};
struct bls381_g2 {
  using ML = launch::bls381_launch<g2_curve>;
  static constexpr size_t ELEM = 96, AUTO_THRESHOLD = ECSIMD_BLS381_G2_MSM_AUTO_THRESHOLD;
  static constexpr const char *name = "bls381_g2", *raw_name = "bls381_g2_raw", *flag_stem = "ECSIMD_BLS381_G2", *msm_launch = "bls381_g2_msm launch";
};
// a message put together from a group's names and widths, for bad() and fail()
struct text { char s[200]; operator const char*() const { return s; } };
__attribute__((format(printf, 1, 2))) text textf(const char* fmt, ...) {
  text t; va_list ap;
  va_start(ap, fmt); vsnprintf(t.s, sizeof t.s, fmt, ap); va_end(ap);
  return t;
}
template <class T> bool bls381_schedule_of(size_t n, int bits, int flags, msm_schedule* S) {
  if (flags != ECSIMD_MSM_ALG_AUTO && flags != ECSIMD_MSM_ALG_BUCKETS && flags != ECSIMD_MSM_ALG_LANES) return false;
  const int route = flags != ECSIMD_MSM_ALG_AUTO ? flags : n >= T::AUTO_THRESHOLD ? ECSIMD_MSM_ALG_BUCKETS : ECSIMD_MSM_ALG_LANES;
  if (route == ECSIMD_MSM_ALG_BUCKETS || n == 0) {
    if (!msm_schedule_of(n, bits, ECSIMD_MSM_ALG_BUCKETS, S, 3, T::ELEM)) return false;
    S->plan.route = route;
    return true;
  }
  if (bits < 1 || bits > 256 || n > ECSIMD_MSM_MAX_N) return false;
  *S = msm_schedule();
  S->planes = 3; S->elem = T::ELEM;
  S->plan.route = ECSIMD_MSM_ALG_LANES;
  S->plan.max_chain = launch::MSM_TREE_FAN;
  S->plan.launches = 3 + tree_passes(n);                              // zero, the products, the tree's passes, the last kernel
  S->plan.workspace_bytes = 16 + 3 * T::ELEM * n;
  return true;
}
template <class T> struct bls381_sum {
  using ML = typename T::ML;
  static constexpr const char* what = T::msm_launch;
  const uint64_t* k; const uint8_t* pts; uint8_t* out;
  void digits(hipStream_t s, const msm_blocks& B, size_t n, int bits, int c, int windows) const { ML::digits(s, k, pts, B.kk, B.px, B.py, B.hist, B.counter, n, bits, c, windows); }
  void slices(hipStream_t s, const msm_blocks& B, size_t n, size_t T_, size_t L, size_t slices, int c, size_t K) const {
    ML::slices(s, B.sorted, B.kk, B.px, B.py, B.start, B.buckets, B.partial, B.counter + 1, n, T_, L, slices, c, K);
  }
  void finish(hipStream_t s, const uint64_t* arr, size_t total, size_t stride, int windows, int c, const uint32_t* counter, uint8_t* finite, uint32_t* invalid) const {
    ML::finish(s, arr, total, stride, windows, c, counter, out, finite, invalid);
  }
};
// the counter (16 bytes, zeroed by a kernel) and a Jacobian array of `elements`, from the start of the workspace
struct bls381_tree_layout { uint32_t* counter; uint64_t* tree; size_t bytes; };
template <class T> bls381_tree_layout bls381_tree_plan(void* base, size_t elements) {
  bls381_tree_layout L; carve c = carve_from(base);
  L.counter = static_cast<uint32_t*>(carve_bytes(c, 16)); L.tree = static_cast<uint64_t*>(carve_bytes(c, 3 * T::ELEM * elements));
  L.bytes = c.bytes;
  return L;
}
// the LANES route (k != nullptr: the products of n terms) and the point sum (k == nullptr: the validating affine front over n encodings); n >= 1
template <class T>
int bls381_tree_sum_run(ecsimd_hip_ctx* ctx, const uint64_t* k, const uint8_t* pts, bool compressed, uint8_t* out, uint8_t* finite, uint32_t* invalid, size_t n, int bits) {
  using ML = typename T::ML;
  hipStream_t s = ctx->stream;
  const int fan = launch::MSM_TREE_FAN;
  const size_t elements = k ? n : (n + fan - 1) / fan;
  const int rc = ensure_workspace(ctx, bls381_tree_plan<T>(nullptr, elements).bytes);
  if (rc != ECSIMD_HIP_OK) return rc;
  const bls381_tree_layout L = bls381_tree_plan<T>(ctx->workspace, elements);
  launch::msm_zero(s, L.counter, 16);
  if (k) ML::products(s, k, pts, L.counter, L.tree, n, bits);
  else ML::tree_affine(s, pts, compressed, L.counter, L.tree, n, elements, fan);
  tree_run<ML>(s, L.tree, elements, elements, 0, 1);
  ML::finish(s, L.tree, elements, 0, 1, 0, L.counter, out, finite, invalid);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? ECSIMD_HIP_OK : fail(ctx, e, k ? T::msm_launch : textf("%s_point_sum launch", T::name));
}
// every output array against every input array (a null one is no array) and the other outputs, as byte ranges
struct byte_array { const void* p; size_t bytes; };
bool arrays_overlap(std::initializer_list<byte_array> outs, std::initializer_list<byte_array> ins) {
  for (auto a = outs.begin(); a != outs.end(); ++a) {
    for (const byte_array& b : ins) if (ranges_overlap(a->p, a->bytes, b.p, b.bytes)) return true;
    for (auto b = a + 1; b != outs.end(); ++b) if (ranges_overlap(a->p, a->bytes, b->p, b->bytes)) return true;
  }
  return false;
}
// the single result's outputs against each other and against the inputs (in1 may be null)
template <class T> bool bls381_result_overlaps(const uint8_t* out, const uint8_t* finite, const uint32_t* invalid, const void* in0, size_t in0_bytes, const void* in1, size_t in1_bytes) {
  return arrays_overlap({{out, 2 * T::ELEM}, {finite, 1}, {invalid, 4}}, {{in0, in0_bytes}, {in1, in1_bytes}});
}
// the entry points' bodies; W, C: the uncompressed and the compressed width in the messages' argument names
#define BLS381_WIDTHS const size_t W = 2 * T::ELEM, C = T::ELEM
#define BLS381_NO_OVERLAP(fn, ...) if (arrays_overlap(__VA_ARGS__)) return bad(ctx, textf("%s_" fn ": an output must not overlap an input or another output", T::name))
#define BLS381_LAUNCHED(fn) const hipError_t e = hipGetLastError(); return e == hipSuccess ? ECSIMD_HIP_OK : fail(ctx, e, textf("%s_" fn " launch", T::name))
template <class T> int bls381_decompress(ecsimd_hip_ctx* ctx, const uint8_t* in, uint8_t* out, uint8_t* ok, size_t n) {
  BLS381_WIDTHS;
  REQUIRE_CTX(); if ((!in || !out || !ok) && n) return bad(ctx, textf("%s_decompress: in%zu, out%zu or ok is null", T::name, C, W));
  BLS381_NO_OVERLAP("decompress", {{out, W * n}, {ok, n}}, {{in, C * n}});
  ENTER();
  T::ML::decompress(ctx->stream, in, out, ok, n);
  BLS381_LAUNCHED("decompress"); }
template <class T> int bls381_compress(ecsimd_hip_ctx* ctx, const uint8_t* in, uint8_t* out, uint8_t* ok, size_t n) {
  BLS381_WIDTHS;
  REQUIRE_CTX(); if ((!in || !out || !ok) && n) return bad(ctx, textf("%s_compress: in%zu, out%zu or ok is null", T::name, W, C));
  BLS381_NO_OVERLAP("compress", {{out, C * n}, {ok, n}}, {{in, W * n}});
  ENTER();
  T::ML::compress(ctx->stream, in, out, ok, n);
  BLS381_LAUNCHED("compress"); }
template <class T> int bls381_check(ecsimd_hip_ctx* ctx, const uint8_t* in, uint8_t* on_curve, uint8_t* in_subgroup, size_t n) {
  BLS381_WIDTHS; (void)C;
  REQUIRE_CTX(); if ((!in || !on_curve || !in_subgroup) && n) return bad(ctx, textf("%s_check: in%zu, on_curve or in_subgroup is null", T::name, W));
  BLS381_NO_OVERLAP("check", {{on_curve, n}, {in_subgroup, n}}, {{in, W * n}});
  ENTER();
  T::ML::check(ctx->stream, in, on_curve, in_subgroup, n);
  BLS381_LAUNCHED("check"); }
template <class T> int bls381_mul(ecsimd_hip_ctx* ctx, const uint64_t* k, const uint8_t* in, uint8_t* out, uint8_t* ok, size_t n) {
  BLS381_WIDTHS; (void)C;
  REQUIRE_CTX(); if ((!k || !in || !out || !ok) && n) return bad(ctx, textf("%s_mul: k, in%zu, out%zu or ok is null", T::name, W, W));
  if (!aligned16(k)) return bad(ctx, textf("%s_mul: k is not 16-byte aligned", T::name));
  BLS381_NO_OVERLAP("mul", {{out, W * n}, {ok, n}}, {{k, 32 * n}, {in, W * n}});
  ENTER();
  T::ML::mul(ctx->stream, k, in, out, ok, n);
  BLS381_LAUNCHED("mul"); }
template <class T> int bls381_msm_plan(size_t n, int bits, int flags, ecsimd_msm_plan_t* out) {
  msm_schedule S;
  if (!out || !bls381_schedule_of<T>(n, bits, flags, &S)) return ECSIMD_HIP_ERR_BAD_ARG;
  *out = S.plan;
  return ECSIMD_HIP_OK; }
template <class T> int bls381_msm(ecsimd_hip_ctx* ctx, const uint64_t* k, const uint8_t* pts, uint8_t* out, uint8_t* finite, uint32_t* invalid, size_t n, int bits, int flags) {
  BLS381_WIDTHS; (void)C;
  REQUIRE_CTX();
  if ((!k || !pts) && n) return bad(ctx, textf("%s_msm: k or pts%zu is null", T::name, W));
  if (!out || !finite) return bad(ctx, textf("%s_msm: out%zu or finite is null", T::name, W));
  if (!aligned16(k)) return bad(ctx, textf("%s_msm: k is not 16-byte aligned", T::name));
  if (invalid && (reinterpret_cast<uintptr_t>(invalid) & 3u)) return bad(ctx, textf("%s_msm: invalid is not 4-byte aligned", T::name));
  if (bits < 1 || bits > 256) return bad(ctx, textf("%s_msm: bits must be 1 .. 256", T::name));
  if (n > ECSIMD_MSM_MAX_N) return bad(ctx, textf("%s_msm: n is above ECSIMD_MSM_MAX_N: chain chunks through ecsimd_%s_point_sum", T::name, T::name));
  msm_schedule S;
  if (!bls381_schedule_of<T>(n, bits, flags, &S)) return bad(ctx, textf("%s_msm: flags must be ECSIMD_MSM_ALG_AUTO, ECSIMD_MSM_ALG_BUCKETS or ECSIMD_MSM_ALG_LANES", T::name));
  if (bls381_result_overlaps<T>(out, finite, invalid, k, 32 * n, pts, W * n)) return bad(ctx, textf("%s_msm: an output must not overlap an input or another output", T::name));
  const hipError_t e0 = hipSetDevice(ctx->device); if (e0 != hipSuccess) return fail(ctx, e0, "hipSetDevice");
  if (n == 0 || S.plan.route == ECSIMD_MSM_ALG_BUCKETS) return bucket_sum_run(ctx, S, bls381_sum<T>{k, pts, out}, finite, invalid, n, bits, 0);
  return bls381_tree_sum_run<T>(ctx, k, pts, false, out, finite, invalid, n, bits); }
// uncompressed_flag, compressed_flag: the group's two encoding flags (the headers give both groups the same values under their own names)
template <class T> int bls381_point_sum(ecsimd_hip_ctx* ctx, const uint8_t* pts, uint8_t* out, uint8_t* finite, uint32_t* invalid, size_t n, int flags, int uncompressed_flag,
                                        int compressed_flag) {
  BLS381_WIDTHS;
  REQUIRE_CTX();
  if (!pts && n) return bad(ctx, textf("%s_point_sum: pts is null", T::name));
  if (!out || !finite) return bad(ctx, textf("%s_point_sum: out%zu or finite is null", T::name, W));
  if (invalid && (reinterpret_cast<uintptr_t>(invalid) & 3u)) return bad(ctx, textf("%s_point_sum: invalid is not 4-byte aligned", T::name));
  if (flags != uncompressed_flag && flags != compressed_flag) return bad(ctx, textf("%s_point_sum: flags must be %s_UNCOMPRESSED or %s_COMPRESSED", T::name, T::flag_stem, T::flag_stem));
  const bool compressed = flags == compressed_flag;
  if ((n + launch::MSM_TREE_FAN - 1) / launch::MSM_TREE_FAN > MAX_LAUNCH) return bad(ctx, "batch too large");
  if (bls381_result_overlaps<T>(out, finite, invalid, pts, (compressed ? C : W) * n, nullptr, 0)) return bad(ctx, textf("%s_point_sum: an output must not overlap an input or another output", T::name));
  const hipError_t e0 = hipSetDevice(ctx->device); if (e0 != hipSuccess) return fail(ctx, e0, "hipSetDevice");
  if (n == 0) return bucket_sum_run(ctx, msm_schedule(), bls381_sum<T>{nullptr, nullptr, out}, finite, invalid, 0, 1, 0);     // the empty sum: the last kernel alone
  return bls381_tree_sum_run<T>(ctx, nullptr, pts, compressed, out, finite, invalid, n, 0); }
template <class T> int bls381_raw_records(int op, bool outputs) {
  const int R = (int)(T::ELEM / 48);
  return (op < 0 || op > launch::BLS381_RAW_POINT_MADD) ? 0 : outputs ? launch::bls381_raw_outputs(op, R) : launch::bls381_raw_inputs(op, R);
}
template <class T> int bls381_raw(ecsimd_hip_ctx* ctx, int op, const uint8_t* in, uint8_t* out, size_t n) {
  REQUIRE_CTX(); if ((!in || !out) && n) return bad(ctx, textf("%s: null pointer", T::raw_name));
  if (op < 0 || op > launch::BLS381_RAW_POINT_MADD) return bad(ctx, textf("%s: unknown function", T::raw_name));
  if (ranges_overlap(in, 48 * (size_t)bls381_raw_records<T>(op, false) * n, out, 48 * (size_t)bls381_raw_records<T>(op, true) * n)) return bad(ctx, textf("%s: out must not overlap in", T::raw_name));
  ENTER();
  T::ML::raw(ctx->stream, op, in, out, n);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? ECSIMD_HIP_OK : fail(ctx, e, textf("%s launch", T::raw_name)); }
#undef BLS381_WIDTHS
#undef BLS381_NO_OVERLAP
#undef BLS381_LAUNCHED
}  // namespace
}  // extern "C++"

int ecsimd_bls12_381_g1_decompress(ecsimd_hip_ctx* ctx, const uint8_t* in48, uint8_t* out96, uint8_t* ok, size_t n) { return bls381_decompress<bls381_g1>(ctx, in48, out96, ok, n); }
int ecsimd_bls12_381_g1_compress(ecsimd_hip_ctx* ctx, const uint8_t* in96, uint8_t* out48, uint8_t* ok, size_t n) { return bls381_compress<bls381_g1>(ctx, in96, out48, ok, n); }
int ecsimd_bls12_381_g1_check(ecsimd_hip_ctx* ctx, const uint8_t* in96, uint8_t* on_curve, uint8_t* in_subgroup, size_t n) { return bls381_check<bls381_g1>(ctx, in96, on_curve, in_subgroup, n); }
int ecsimd_bls12_381_g1_mul(ecsimd_hip_ctx* ctx, const uint64_t* k, const uint8_t* in96, uint8_t* out96, uint8_t* ok, size_t n) { return bls381_mul<bls381_g1>(ctx, k, in96, out96, ok, n); }
int ecsimd_bls12_381_g1_msm_plan(size_t n, int bits, int flags, ecsimd_msm_plan_t* out) { return bls381_msm_plan<bls381_g1>(n, bits, flags, out); }
int ecsimd_bls12_381_g1_msm(ecsimd_hip_ctx* ctx, const uint64_t* k, const uint8_t* pts96, uint8_t* out96, uint8_t* finite, uint32_t* invalid, size_t n, int bits, int flags) {
  return bls381_msm<bls381_g1>(ctx, k, pts96, out96, finite, invalid, n, bits, flags); }
int ecsimd_bls12_381_g1_point_sum(ecsimd_hip_ctx* ctx, const uint8_t* pts, uint8_t* out96, uint8_t* finite, uint32_t* invalid, size_t n, int flags) {
  return bls381_point_sum<bls381_g1>(ctx, pts, out96, finite, invalid, n, flags, ECSIMD_BLS12_381_UNCOMPRESSED, ECSIMD_BLS12_381_COMPRESSED); }
int ecsimd_bls12_381_raw_inputs(int op) { return bls381_raw_records<bls381_g1>(op, false); }
int ecsimd_bls12_381_raw_outputs(int op) { return bls381_raw_records<bls381_g1>(op, true); }
int ecsimd_bls12_381_raw(ecsimd_hip_ctx* ctx, int op, const uint8_t* in, uint8_t* out, size_t n) { return bls381_raw<bls381_g1>(ctx, op, in, out, n); }

int ecsimd_bls381_g2_decompress(ecsimd_hip_ctx* ctx, const uint8_t* in96, uint8_t* out192, uint8_t* ok, size_t n) { return bls381_decompress<bls381_g2>(ctx, in96, out192, ok, n); }
int ecsimd_bls381_g2_compress(ecsimd_hip_ctx* ctx, const uint8_t* in192, uint8_t* out96, uint8_t* ok, size_t n) { return bls381_compress<bls381_g2>(ctx, in192, out96, ok, n); }
int ecsimd_bls381_g2_check(ecsimd_hip_ctx* ctx, const uint8_t* in192, uint8_t* on_curve, uint8_t* in_subgroup, size_t n) { return bls381_check<bls381_g2>(ctx, in192, on_curve, in_subgroup, n); }
int ecsimd_bls381_g2_mul(ecsimd_hip_ctx* ctx, const uint64_t* k, const uint8_t* in192, uint8_t* out192, uint8_t* ok, size_t n) { return bls381_mul<bls381_g2>(ctx, k, in192, out192, ok, n); }
int ecsimd_bls381_g2_msm_plan(size_t n, int bits, int flags, ecsimd_msm_plan_t* out) { return bls381_msm_plan<bls381_g2>(n, bits, flags, out); }
int ecsimd_bls381_g2_msm(ecsimd_hip_ctx* ctx, const uint64_t* k, const uint8_t* pts192, uint8_t* out192, uint8_t* finite, uint32_t* invalid, size_t n, int bits, int flags) {
  return bls381_msm<bls381_g2>(ctx, k, pts192, out192, finite, invalid, n, bits, flags); }
int ecsimd_bls381_g2_point_sum(ecsimd_hip_ctx* ctx, const uint8_t* pts, uint8_t* out192, uint8_t* finite, uint32_t* invalid, size_t n, int flags) {
  return bls381_point_sum<bls381_g2>(ctx, pts, out192, finite, invalid, n, flags, ECSIMD_BLS381_G2_UNCOMPRESSED, ECSIMD_BLS381_G2_COMPRESSED); }
int ecsimd_bls381_g2_raw_inputs(int op) { return bls381_raw_records<bls381_g2>(op, false); }
int ecsimd_bls381_g2_raw_outputs(int op) { return bls381_raw_records<bls381_g2>(op, true); }
int ecsimd_bls381_g2_raw(ecsimd_hip_ctx* ctx, int op, const uint8_t* in, uint8_t* out, size_t n) { return bls381_raw<bls381_g2>(ctx, op, in, out, n); }

int ecsimd_ed25519_verify_cofactored(ecsimd_hip_ctx* ctx, const uint8_t* pk, const uint8_t* msg, size_t msg_bytes, size_t stride_bytes, const uint32_t* lens,
                                     const uint8_t* sig, uint8_t* ok, size_t n, int flags) {
  REQUIRE_CTX(); if ((!pk || !sig || !ok) && n) return bad(ctx, "ed25519_verify_cofactored: pk, sig or ok is null");
  if (flags & ~ECSIMD_ED25519_REJECT_SMALL_ORDER) return bad(ctx, "ed25519_verify_cofactored: unknown flag");
  int rc = ed25519_messages(ctx, msg, &msg_bytes, stride_bytes, lens, n); if (rc != ECSIMD_HIP_OK) return rc;
  if (n != 0 && any_alias({ok}, {pk, msg, sig, lens})) return bad(ctx, "ed25519_verify_cofactored: ok must not alias an input");
  ENTER_ANY_SIZE();
  rc = edc_run(ctx, pk, msg, msg_bytes, stride_bytes, lens, sig, ok, n, (flags & ECSIMD_ED25519_REJECT_SMALL_ORDER) != 0, nullptr); if (rc != ECSIMD_HIP_OK) return rc;
  const hipError_t err = hipGetLastError();
  return err == hipSuccess ? ECSIMD_HIP_OK : fail(ctx, err, "ed25519_verify_cofactored launch"); }

int ecsimd_ed25519_batch_plan(size_t n, size_t msg_bytes, int flags, ecsimd_ed25519_batch_plan_t* out) {
  edb_schedule S;
  if (!out || !edb_schedule_of(n, msg_bytes, flags, &S)) return ECSIMD_HIP_ERR_BAD_ARG;
  *out = S.plan;
  return ECSIMD_HIP_OK; }

int ecsimd_ed25519_verify_batch(ecsimd_hip_ctx* ctx, const uint8_t* pk, const uint8_t* msg, size_t msg_bytes, size_t stride_bytes, const uint32_t* lens,
                                const uint8_t* sig, uint8_t* ok, size_t n, int flags) {
  REQUIRE_CTX();
  if (!ok) return bad(ctx, "ed25519_verify_batch: ok is null");
  if (!edb_flags_ok(flags)) return bad(ctx, "ed25519_verify_batch: flags must be ECSIMD_ED25519_BATCH_AUTO, _MSM or _LANES, or-able with ECSIMD_ED25519_REJECT_SMALL_ORDER");
  int rc = edb_check(ctx, pk, msg, &msg_bytes, stride_bytes, lens, sig, ok, 1, n); if (rc != ECSIMD_HIP_OK) return rc;
  edb_schedule S;
  if (!edb_schedule_of(n, lens ? stride_bytes : msg_bytes, flags, &S)) return bad(ctx, "ed25519_verify_batch: no schedule for these arguments");
  const hipError_t e0 = hipSetDevice(ctx->device); if (e0 != hipSuccess) return fail(ctx, e0, "hipSetDevice");
  hipStream_t s = ctx->stream;
  if (n == 0) launch::flags_all(s, nullptr, 0, ok);
  else if (S.plan.route == ECSIMD_ED25519_BATCH_LANES) {
    uint8_t* verdicts = nullptr;
    rc = edc_run(ctx, pk, msg, msg_bytes, stride_bytes, lens, sig, nullptr, n, S.reject_small, &verdicts); if (rc != ECSIMD_HIP_OK) return rc;
    launch::flags_all(s, verdicts, n, ok);
  } else {
    rc = ensure_workspace(ctx, S.plan.workspace_bytes); if (rc != ECSIMD_HIP_OK) return rc;      // all of it now: the sums below find it large enough, nothing moves
    size_t own = 0;
    const edb_blocks B = edb_carve(n, ctx->workspace, &own);
    edb_randomizers(ctx, B, pk, msg, msg_bytes, stride_bytes, lens, sig, S.reject_small, B.z, true, n);
    batch_scalar_sum(B.zs, B.sums, B.zh + 4 * n, n, [&](const uint64_t* in, size_t count, uint64_t* out, bool last) {        // sum z s, and B's encoding beside it
      launch::ed25519_batch_sum(s, *ed25519_order(), in, count, out, last ? B.Aenc + 4 * n : nullptr);
    });
    rc = bucket_sum_run(ctx, S.sums.r, edwards_sum{reinterpret_cast<const uint8_t*>(B.z), reinterpret_cast<const uint8_t*>(B.Renc), nullptr, B.head->sum[0]}, &B.head->finite[0],
                        &B.head->invalid[0], n, 128, own);
    if (rc == ECSIMD_HIP_OK) rc = bucket_sum_run(ctx, S.sums.key, edwards_sum{reinterpret_cast<const uint8_t*>(B.zh), reinterpret_cast<const uint8_t*>(B.Aenc), nullptr, B.head->sum[1]},
                                                 &B.head->finite[1], &B.head->invalid[1], n + 1, EDB_KEY_BITS, own);
    if (rc != ECSIMD_HIP_OK) return rc;
    launch::ed25519_batch_accept(s, B.head, ok);
  }
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? ECSIMD_HIP_OK : fail(ctx, e, "ed25519_verify_batch launch"); }

int ecsimd_ed25519_batch_randomizers(ecsimd_hip_ctx* ctx, const uint8_t* pk, const uint8_t* msg, size_t msg_bytes, size_t stride_bytes, const uint32_t* lens,
                                     const uint8_t* sig, uint8_t* z, size_t n) {
  REQUIRE_CTX();
  if (!z && n) return bad(ctx, "ed25519_batch_randomizers: z is null");
  if (!aligned16(z)) return bad(ctx, "ed25519_batch_randomizers: z is not 16-byte aligned");
  int rc = edb_check(ctx, pk, msg, &msg_bytes, stride_bytes, lens, sig, z, 32 * n, n); if (rc != ECSIMD_HIP_OK) return rc;
  ENTER_ANY_SIZE();
  size_t own = 0;
  (void)edb_carve(n, nullptr, &own);
  rc = ensure_workspace(ctx, own); if (rc != ECSIMD_HIP_OK) return rc;
  edb_randomizers(ctx, edb_carve(n, ctx->workspace, &own), pk, msg, msg_bytes, stride_bytes, lens, sig, false, reinterpret_cast<uint64_t*>(z), false, n);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? ECSIMD_HIP_OK : fail(ctx, e, "ed25519_batch_randomizers launch"); }

int ecsimd_hip_fe29_raw(ecsimd_hip_ctx* ctx, int curve, int op, const int32_t* in, int32_t* out, size_t n, int swap) {
  REQUIRE_CTX(); if ((!in || !out) && n) return bad(ctx, "fe29_raw: null pointer");
  if (op < 0 || op > launch::RAW_ZADDU) return bad(ctx, "fe29_raw: unknown function");
  gcurve GC; const bool registered = curve >= ECSIMD_HIP_FIRST_REGISTERED_CURVE;
  if (registered) { if (!lookup_curve(curve, &GC)) return bad(ctx, "unknown curve id"); }
  else REQUIRE_CURVE();
  ENTER();
  if (!launch::fe29_raw(ctx->stream, registered ? 2 : curve, registered ? &GC : nullptr, op, in, out, n, swap ? 0xffffffffu : 0u)) return bad(ctx, "fe29_raw: this function does not exist for this curve");
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? ECSIMD_HIP_OK : fail(ctx, e, "fe29_raw launch"); }

int ecsimd_hip_workspace_info(ecsimd_hip_ctx* ctx, const void** dptr, size_t* bytes) {
  REQUIRE_CTX(); if (!dptr || !bytes) return bad(ctx, "workspace_info: null output");
  *dptr = ctx->workspace; *bytes = ctx->workspace_bytes; return ECSIMD_HIP_OK; }

int ecsimd_hip_scalar_mult_p256(ecsimd_hip_ctx* ctx, const uint64_t* k, const uint64_t* xm, const uint64_t* ym, uint64_t* ox, uint64_t* oy, uint64_t* oz, size_t n) {
  return ecsimd_hip_scalar_mult(ctx, ECSIMD_HIP_P256, k, xm, ym, ox, oy, oz, n, ECSIMD_HIP_BASE_MGRY | ECSIMD_HIP_OUT_JACOBIAN); }

int ecsimd_hip_fill_random(ecsimd_hip_ctx* ctx, uint64_t* out, size_t n, uint64_t seed, uint64_t stream, uint64_t first_index, int clear_top_bits) {
  REQUIRE_CTX(); REQUIRE_PTR(out); if (clear_top_bits < 0 || clear_top_bits > 63) return bad(ctx, "clear_top_bits");
  RUN(launch::fill_random(s, out, n, seed, stream, first_index, clear_top_bits)); }

int ecsimd_hip_peak_mad32(ecsimd_hip_ctx* ctx, int iters, double* mads, double* ms) {
  REQUIRE_CTX(); if (iters < 1 || !mads || !ms) return bad(ctx, "peak_mad32 arguments");
  REFUSE_IN_CAPTURE("peak_mad32 times its launches with events and waits for them");
  (void)hipSetDevice(ctx->device);
  const int blocks = ctx->cus * 8;          // 8 workgroups of 4 waves per CU = 8 waves per SIMD
  hipEvent_t e0, e1; (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
  launch::peak_mad32(ctx->stream, blocks, ctx->sink, 16, 1u);   // warm-up
  (void)hipEventRecord(e0, ctx->stream);
  launch::peak_mad32(ctx->stream, blocks, ctx->sink, iters, 2u);
  (void)hipEventRecord(e1, ctx->stream);
  hipError_t e = hipEventSynchronize(e1);
  float t = 0; if (e == hipSuccess) e = hipEventElapsedTime(&t, e0, e1);
  (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
  if (e != hipSuccess) return fail(ctx, e, "peak_mad32");
  *ms = t; *mads = (double)blocks * BLOCK * (double)iters * launch::PEAK_MADS_PER_LANE_PER_ITER;
  return ECSIMD_HIP_OK; }


// ---- SHA-512, HMAC-SHA-512 (k_sha512.hip); public data, no workspace
int ecsimd_hip_sha512(ecsimd_hip_ctx* ctx, const uint8_t* msg, size_t msg_bytes, size_t stride_bytes, uint8_t* out64, size_t n) {
  REQUIRE_CTX();
  int rc = btc_hash_args(ctx, "sha512", msg, msg_bytes, stride_bytes, out64, n); if (rc != ECSIMD_HIP_OK) return rc;
  if (!aligned16(out64)) return bad(ctx, "out64 is not 16-byte aligned");
  RUN(launch::sha512(s, msg, msg_bytes, stride_bytes, out64, n)); }

int ecsimd_hip_hmac_sha512(ecsimd_hip_ctx* ctx, const uint8_t* key, size_t key_bytes, size_t key_stride_bytes, const uint8_t* msg, size_t msg_bytes, size_t stride_bytes,
                           uint8_t* out64, size_t n) {
  REQUIRE_CTX();
  int rc = btc_hash_args(ctx, "hmac_sha512", msg, msg_bytes, stride_bytes, out64, n); if (rc != ECSIMD_HIP_OK) return rc;
  if (!aligned16(out64)) return bad(ctx, "out64 is not 16-byte aligned");
  if (!key && n && key_bytes) return bad(ctx, "key is null");
  if ((key_stride_bytes != 0 && key_stride_bytes < key_bytes) || key_bytes > ((size_t)1 << 40)) return bad(ctx, "hmac_sha512: key_stride_bytes is smaller than key_bytes, or the key is too long");
  RUN(launch::hmac_sha512(s, key, key_bytes, key_stride_bytes, msg, msg_bytes, stride_bytes, out64, n)); }

// ---- BIP-32 key derivation on secp256k1 (k_bip32.hip)
namespace {
int bip32_common(ecsimd_hip_ctx* ctx, const char* what, const uint32_t* index, group_order* O) {
  if (reinterpret_cast<uintptr_t>(index) & 3u) return bad(ctx, "index is not 4-byte aligned");
  if (wants_compat(ctx)) return refuse_compat(ctx, what);
  return builtin_order(ctx, ECSIMD_HIP_SECP256K1, O);
}
}  // namespace

int ecsimd_hip_bip32_master(ecsimd_hip_ctx* ctx, const uint8_t* seed, size_t seed_bytes, size_t stride_bytes, uint64_t* k, uint64_t* c, uint8_t* ok, size_t n) {
  REQUIRE_CTX(); REQUIRE_PTR(k); REQUIRE_PTR(c);
  if ((!ok || !seed) && n) return bad(ctx, "seed or ok is null");
  if (seed_bytes < 16 || seed_bytes > 64) return bad(ctx, "bip32_master: seed_bytes is outside 16 .. 64");
  if (stride_bytes < seed_bytes) return bad(ctx, "bip32_master: stride_bytes is smaller than seed_bytes");
  group_order O;
  int rc = bip32_common(ctx, "bip32_master", nullptr, &O); if (rc != ECSIMD_HIP_OK) return rc;
  if (n != 0 && any_alias({k, c, ok}, {seed})) return bad(ctx, "k, c and ok must not alias an input or each other");
  RUN(launch::bip32_master(s, O.words, seed, seed_bytes, stride_bytes, k, c, ok, n)); }

// Without the caller's promise, per chunk of 2^22: k_par G on the constant-time comb with both coordinates through the simultaneous inversion
// (secret_base_product), then k_bip32_ckd_priv<true>.  Per element of a chunk: the Jacobian product (96 B) and the affine k_par G (64 B) -- all
// zeroed behind the kernels (secret_base_product says why).  With the promise (or index == NULL and a hardened index_all): k_bip32_ckd_priv<false> alone, no workspace.
int ecsimd_hip_bip32_ckd_priv(ecsimd_hip_ctx* ctx, const uint64_t* k_par, const uint64_t* c_par, const uint32_t* index, uint32_t index_all, uint64_t* k_child, uint64_t* c_child,
                              uint8_t* ok, size_t n, int flags) {
  REQUIRE_CTX(); REQUIRE_PTR(k_par); REQUIRE_PTR(c_par); REQUIRE_PTR(k_child); REQUIRE_PTR(c_child);
  if (!ok && n) return bad(ctx, "ok is null");
  if (flags & ~ECSIMD_HIP_BIP32_ALL_HARDENED) return bad(ctx, "bip32_ckd_priv: unknown flag");
  group_order O;
  int rc = bip32_common(ctx, "bip32_ckd_priv", index, &O); if (rc != ECSIMD_HIP_OK) return rc;
  if (n != 0 && any_alias({k_child, c_child, ok}, {k_par, c_par, index})) return bad(ctx, "k_child, c_child and ok must not alias an input or each other");
  const int curve = ECSIMD_HIP_SECP256K1;
  hipError_t err = hipSuccess;
  if ((flags & ECSIMD_HIP_BIP32_ALL_HARDENED) != 0 || (!index && (index_all >> 31) != 0)) {      // hardened only -- no workspace: nothing to chunk
    ENTER();
    launch::bip32_ckd_priv(ctx->stream, O.N, k_par, c_par, index, index_all, nullptr, nullptr, k_child, c_child, ok, n);
    err = hipGetLastError();
    return err == hipSuccess ? ECSIMD_HIP_OK : fail(ctx, err, "bip32_ckd_priv launch");
  }
  ENTER_ANY_SIZE();
  const size_t chunk = chunk_of(n, GC_CHUNK);
  rc = ensure_window_table(ctx, curve, CT_WBITS);
  if (rc == ECSIMD_HIP_OK) rc = ensure_workspace(ctx, sign_plan(nullptr, chunk, true).bytes);
  if (rc != ECSIMD_HIP_OK) return rc;
  const sign_layout L = sign_plan(ctx->workspace, chunk, true);              // the Jacobian k_par G and both affine coordinates
  FOR_CHUNKS(first, m, n, chunk) {
    secret_base_product(ctx, curve, k_par + 4 * first, L.j, L.rx, L.ry, m);
    launch::bip32_ckd_priv(ctx->stream, O.N, k_par + 4 * first, c_par + 4 * first, index ? index + first : nullptr, index_all, L.rx, L.ry, k_child + 4 * first, c_child + 4 * first, ok + first, m);
    err = wipe_workspace(ctx, L.bytes, hipGetLastError());
    if (err != hipSuccess) break;
  }
  return err == hipSuccess ? ECSIMD_HIP_OK : fail(ctx, err, "bip32_ckd_priv launch"); }

// (cx, cy) = IL G + K per chunk of 2^22: k_bip32_ckd_pub_front (the hash, the curve equation, the range checks), then tweak_middle -- IL G on the
// public comb, k_tweak_add, ONE simultaneous inversion that keeps y --, then k_bip32_ckd_pub_accept.  Per element of a chunk: K, later the affine sum (64 B),
// IL (32 B), the Jacobian sum (96 B) and the validity byte.  The child chain code goes straight to its output.
int ecsimd_hip_bip32_ckd_pub(ecsimd_hip_ctx* ctx, const uint64_t* qx, const uint64_t* qy, const uint64_t* c_par, const uint32_t* index, uint32_t index_all, uint64_t* cx, uint64_t* cy,
                             uint64_t* c_child, uint8_t* ok, size_t n) {
  REQUIRE_CTX(); REQUIRE_PTR(qx); REQUIRE_PTR(qy); REQUIRE_PTR(c_par); REQUIRE_PTR(cx); REQUIRE_PTR(cy); REQUIRE_PTR(c_child);
  if (!ok && n) return bad(ctx, "ok is null");
  group_order O;
  int rc = bip32_common(ctx, "bip32_ckd_pub", index, &O); if (rc != ECSIMD_HIP_OK) return rc;
  if (n != 0 && any_alias({cx, cy, c_child, ok}, {qx, qy, c_par, index})) return bad(ctx, "cx, cy, c_child and ok must not alias an input or each other");
  ENTER_ANY_SIZE();
  tweak_layout L; rc = tweak_prepare(ctx, n, &L);
  if (rc != ECSIMD_HIP_OK) return rc;
  FOR_CHUNKS(first, m, n, L.chunk) {
    launch::bip32_ckd_pub_front(ctx->stream, O.words, qx + 4 * first, qy + 4 * first, c_par + 4 * first, index ? index + first : nullptr, index_all, L.x, L.y, L.t, c_child + 4 * first, L.valid, m);
    tweak_middle(ctx, n, L, m);
    launch::bip32_ckd_pub_accept(ctx->stream, L.x, L.y, L.j.z, L.valid, cx + 4 * first, cy + 4 * first, c_child + 4 * first, ok + first, m);
  }
  hipError_t err = hipGetLastError();
  return err == hipSuccess ? ECSIMD_HIP_OK : fail(ctx, err, "bip32_ckd_pub launch"); }

// ---- PBKDF2-HMAC-SHA-512 and the BIP-39 seed (k_pbkdf2.hip); SECRET contents, PUBLIC lengths
namespace {
// How much one launch may do.  The loop body of k_pbkdf2 is 7 936 VALU instructions per iteration in the shipped listing (profiles/r11/bip39_listing.json) and the
// device issues 35.5 T of them a second (39.3 T a priori, 35.2 .. 35.9 T read by ecsimd_hip_peak_mad32), which predicted 2^29 x 7 936 / 35.5 T =
// 0.12 s for a launch of PBKDF2_UNIT_ITERATIONS = 2^29 (unit, iteration) pairs.  MEASURED on an MI355X (profiles/r11/bip39.txt): 109.7 ms for BIP-39's launch of 2^18
// lanes x 2 048 iterations.  A unit is one 64-byte output block of one lane.  ECSIMD_HIP_PBKDF2_SLICE = 4 096 iterations bounds a launch of few units (65 lanes:
// predicted 4 096 x 7 936 x 4 cycles at 2.4 GHz = 54 ms, measured 57.0 ms) and is twice BIP-39's count, so that c = 2 048 is ONE launch per chunk without the
// workspace; PBKDF2_UNITS = 2^18 is 2^29 / 2 048, BIP-39's chunk, and two full residencies of the device at the kernel's two waves per SIMD (256 CUs x 4 SIMDs x
// 2 waves x 64 lanes = 2^17).  From 4 096 iterations on a launch has 2^17 units: one residency.
constexpr size_t PBKDF2_UNITS = (size_t)1 << 18;
constexpr size_t PBKDF2_UNIT_ITERATIONS = (size_t)1 << 29;
constexpr size_t PBKDF2_MAX_BYTES = (size_t)1 << 30;              // of a password, a salt, a derived key: lengths are 32-bit in the kernel
static_assert(PBKDF2_UNIT_ITERATIONS / ECSIMD_HIP_PBKDF2_SLICE >= 1 && PBKDF2_UNIT_ITERATIONS / PBKDF2_UNITS <= ECSIMD_HIP_PBKDF2_SLICE, "the chunk is never empty and BIP-39's is PBKDF2_UNITS");
struct pbkdf2_layout { void* state; size_t bytes; };              // inner midstate, outer midstate, U, T: 256 B per unit of a sliced derivation
pbkdf2_layout pbkdf2_plan(void* base, size_t units) {
  pbkdf2_layout L; carve c = carve_from(base);
  L.state = carve_bytes(c, units * 256); L.bytes = c.bytes;
  return L;
}
// n byte strings as the call takes its passwords and its salts: lane i's at p + i * stride, lens[i] bytes of it (at most stride), or `bytes` where lens == NULL
struct byte_rows { const uint8_t* p; size_t bytes, stride; const uint32_t* lens; };
int pbkdf2_rows(ecsimd_hip_ctx* ctx, const char* what, byte_rows& r, size_t n, bool one_for_all) {
  if (r.lens) r.bytes = 0;                                                          // (ignored: every lane has its own length)
  const bool shared = one_for_all && r.stride == 0;
  const char* wrong = nullptr;
  if (!r.p && n && (r.bytes || (r.lens && r.stride))) wrong = "is null";
  else if (reinterpret_cast<uintptr_t>(r.lens) & 3u) wrong = "has lens that are not 4-byte aligned";
  else if (shared && r.lens) wrong = "has stride 0 (one for the call) and lens";
  else if (!shared && r.stride < r.bytes) wrong = "has a stride smaller than its length";
  else if (r.bytes > PBKDF2_MAX_BYTES || (r.lens && r.stride > PBKDF2_MAX_BYTES)) wrong = "is too long (with lens, a lane may be as long as the stride)";
  if (!wrong) return ECSIMD_HIP_OK;
  snprintf(ctx->err, sizeof ctx->err, "bad argument: pbkdf2_hmac_sha512: the %s %s", what, wrong);
  return ECSIMD_HIP_ERR_BAD_ARG;
}
byte_rows rows_from(const byte_rows& r, size_t first) { byte_rows q = r; if (q.p) q.p += first * q.stride; if (q.lens) q.lens += first; return q; }

// The derivation behind both entry points.  pre: pre_bytes (0 or 8) bytes in front of every salt.  Lanes in chunks and output blocks in groups of at most
// PBKDF2_UNITS units and PBKDF2_UNIT_ITERATIONS per launch; the iterations of a unit in slices of ECSIMD_HIP_PBKDF2_SLICE, between which its four states lie in
// the workspace -- zeroed behind the last slice whatever the launches said.  iterations <= ECSIMD_HIP_PBKDF2_SLICE: one launch per chunk, no workspace.
int pbkdf2_derive(ecsimd_hip_ctx* ctx, byte_rows pw, byte_rows salt, uint64_t pre, unsigned pre_bytes, uint32_t iterations, uint8_t* out, size_t dk_bytes, size_t out_stride_bytes, size_t n) {
  int rc = pbkdf2_rows(ctx, "password", pw, n, false); if (rc != ECSIMD_HIP_OK) return rc;
  rc = pbkdf2_rows(ctx, "salt", salt, n, true); if (rc != ECSIMD_HIP_OK) return rc;
  if (iterations < 1 || dk_bytes < 1 || dk_bytes > PBKDF2_MAX_BYTES) return bad(ctx, "pbkdf2_hmac_sha512: iterations and dk_bytes are at least 1 (dk_bytes at most 2^30)");
  if (out_stride_bytes < dk_bytes) return bad(ctx, "pbkdf2_hmac_sha512: out_stride_bytes is smaller than dk_bytes");
  if (!out && n) return bad(ctx, "the output is null");
  if (n != 0 && any_alias({out}, {pw.p, salt.p, pw.lens, salt.lens})) return bad(ctx, "out must not alias an input");
  ENTER_ANY_SIZE();
  const size_t slice = ECSIMD_HIP_PBKDF2_SLICE, blocks = (dk_bytes + 63) / 64;
  const size_t most = chunk_of(PBKDF2_UNITS, PBKDF2_UNIT_ITERATIONS / chunk_of(iterations, slice));
  const size_t chunk = chunk_of(n, most), group = chunk_of(blocks, chunk_of(most / chunk, 1u << 15));      // (a grid's y is below 2^16)
  const bool sliced = iterations > slice;
  pbkdf2_layout L = pbkdf2_plan(nullptr, 0);
  if (sliced) {
    rc = ensure_workspace(ctx, pbkdf2_plan(nullptr, chunk * group).bytes);
    if (rc != ECSIMD_HIP_OK) return rc;
    L = pbkdf2_plan(ctx->workspace, chunk * group);
  }
  hipError_t err = hipSuccess;
  FOR_CHUNKS(first, m, n, chunk) {
    const byte_rows P = rows_from(pw, first), S = rows_from(salt, first);
    FOR_CHUNKS(block, nb, blocks, group) {
      for (size_t done = 0, take; done < iterations; done += take) {
        take = chunk_of(iterations - done, slice);
        launch::pbkdf2_hmac_sha512(ctx->stream, done == 0, done + take == iterations, P.p, P.bytes, P.stride, P.lens, S.p, S.bytes, S.stride, S.lens, pre, pre_bytes, (unsigned)block,
                                   (unsigned)nb, (unsigned)(done == 0 ? take - 1 : take), L.state, out + first * out_stride_bytes, dk_bytes, out_stride_bytes, m);
      }
      err = sliced ? wipe_workspace(ctx, L.bytes, hipGetLastError()) : hipGetLastError();
      if (err != hipSuccess) break;
    }
    if (err != hipSuccess) break;
  }
  return err == hipSuccess ? ECSIMD_HIP_OK : fail(ctx, err, "pbkdf2_hmac_sha512 launch");
}
}  // namespace

// (ECSIMD_HIP_REF_SQUARE_COMPAT concerns curve arithmetic: there is none here, so a context with that option is served like any other)
int ecsimd_hip_pbkdf2_hmac_sha512(ecsimd_hip_ctx* ctx, const uint8_t* pw, size_t pw_bytes, size_t pw_stride_bytes, const uint32_t* pw_lens, const uint8_t* salt, size_t salt_bytes,
                                  size_t salt_stride_bytes, const uint32_t* salt_lens, uint32_t iterations, uint8_t* out, size_t dk_bytes, size_t out_stride_bytes, size_t n) {
  REQUIRE_CTX();
  return pbkdf2_derive(ctx, {pw, pw_bytes, pw_stride_bytes, pw_lens}, {salt, salt_bytes, salt_stride_bytes, salt_lens}, 0u, 0u, iterations, out, dk_bytes, out_stride_bytes, n); }

// salt = "mnemonic" || passphrase: the eight bytes are ONE block word, handed to the kernel by value
int ecsimd_hip_bip39_seed(ecsimd_hip_ctx* ctx, const uint8_t* mnemonic, size_t mnemonic_bytes, size_t mnemonic_stride_bytes, const uint32_t* mnemonic_lens, const uint8_t* passphrase,
                          size_t passphrase_bytes, size_t passphrase_stride_bytes, const uint32_t* passphrase_lens, uint8_t* seed64, size_t n) {
  REQUIRE_CTX();
  return pbkdf2_derive(ctx, {mnemonic, mnemonic_bytes, mnemonic_stride_bytes, mnemonic_lens}, {passphrase, passphrase_bytes, passphrase_stride_bytes, passphrase_lens},
                       0x6d6e656d6f6e6963ull /* "mnemonic" */, 8u, 2048u, seed64, 64, 64, n); }
}  // extern "C"

// ================================================================== number-theoretic transform (include/ecsimd_ntt.h)
// ntt.cuh decides the schedule and every index; k_ntt.hip runs one pass per launch.  Here: the host-only questions about a field (two-adicity, roots), a domain's
// tables -- computed on the host with ntt.cuh's portable Montgomery arithmetic, at most 6 x 2^12 + 4 x 2^12 products, and uploaded once -- and the calls' checks.
namespace {
using ntt::pel;
using ntt::pfield;
pfield pfield_of(const gmod& M) {
  pfield F;
  for (int i = 0; i < 8; ++i) { F.p[i] = M.p[i]; F.r2[i] = M.rsq[i]; }
  F.mprime = M.mprime;
  return F;
}
pel pel_of(const uint32_t (&w)[8]) { pel r; for (int i = 0; i < 8; ++i) r.w[i] = w[i]; return r; }
pel pel_of(const u256& v) { pel r; limbs_to_words(v.l, r.w); return r; }
u256 u_of(const pel& v) { u256 r; words_to_limbs(v.w, r.l); return r; }
bool pel_eq(const pel& a, const pel& b) { return !memcmp(a.w, b.w, sizeof a.w); }
pel to_mgry(const pfield& F, const pel& a) { return F.mul(a, F.rsq()); }
pel from_mgry(const pfield& F, const pel& a) { return F.mul(a, pfield::one()); }
// base^e, Montgomery form in and out (one = R mod p)
pel p_pow(const pfield& F, const pel& one, pel base, const u256& e) {
  pel r = one;
  for (int i = 0; i < 256; ++i) {
    if ((e.l[i >> 6] >> (i & 63)) & 1u) r = F.mul(r, base);
    base = F.mul(base, base);
  }
  return r;
}
u256 u_shr(u256 a, int bits) {
  for (; bits > 0; --bits) { for (int i = 0; i < 3; ++i) a.l[i] = (a.l[i] >> 1) | (a.l[i + 1] << 63); a.l[3] >>= 1; }
  return a;
}
// The field of an id, for a transform: a modulus the registry holds as PRIME, a registered curve's prime, or one of the two curve primes.
bool ntt_field(int field, gmod* M) {
  if (field == ECSIMD_HIP_P256 || field == ECSIMD_HIP_SECP256K1) {
    uint64_t c[4];
    words_to_limbs(field == ECSIMD_HIP_P256 ? curve_consts<CURVE_P256>::P : curve_consts<CURVE_SECP256K1>::P, c);
    *M = make_gmod(c, GMOD_PRIME);
    return true;
  }
  return lookup_modulus(field, M) && (M->flags & GMOD_PRIME);
}
struct field_facts { int s; u256 pm1; pel one, minus_one; };       // p - 1 = 2^s m; 1 and -1 in Montgomery form
field_facts facts_of(const gmod& M) {
  field_facts K;
  K.one = pel_of(M.r); K.minus_one = pel_of(M.negr);
  u256 p; words_to_limbs(M.p, p.l);
  const u256 one = {{1, 0, 0, 0}};
  (void)u_sub(K.pm1, p, one);
  K.s = 0;
  while (!((u_shr(K.pm1, K.s).l[0]) & 1u)) ++K.s;                    // p is odd and >= 3: p - 1 is even and not 0
  return K;
}
// g^((p - 1) / 2^s) for the smallest integer g >= 2 with g^((p - 1) / 2) = -1, in Montgomery form
pel default_root_mgry(const pfield& F, const field_facts& K) {
  pel g = F.add(K.one, K.one);
  while (!pel_eq(p_pow(F, K.one, g, u_shr(K.pm1, 1)), K.minus_one)) g = F.add(g, K.one);     // a prime has a non-residue below it
  return p_pow(F, K.one, g, u_shr(K.pm1, K.s));
}
constexpr uint64_t FR_LIMBS[4] = {0xffffffff00000001ull, 0x53bda402fffe5bfeull, 0x3339d80809a1d805ull, 0x73eda753299d7d48ull};
}  // namespace

struct ecsimd_ntt_domain {
  ecsimd_hip_ctx* owner;
  gmod M;
  int log_n, coset;
  ntt::u4* block;                // the tables, one allocation
  ntt::tables tw[2];             // [0] forward, [1] inverse: pointers into block
};

namespace {
int ntt_cap(int flags) {         // the log-radix cap of `flags`, 0 if they are no flags
  if (flags & ~15) return 0;
  const int cap = flags ? flags : ntt::DEFAULT_RADIX_LOG;
  return cap <= ntt::DEFAULT_RADIX_LOG ? cap : 0;
}
constexpr size_t NTT_MAX_ELEMENTS = (size_t)1 << 38;
bool ranges_overlap(const void* a, const void* b, size_t bytes) {
  const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
  return x < y + bytes && y < x + bytes;
}
int ntt_transform(ecsimd_hip_ctx* ctx, const ecsimd_ntt_domain* dom, const uint64_t* in, uint64_t* out, size_t batch, int flags, int inverse) {
  REQUIRE_CTX();
  if (!dom) return bad(ctx, "dom is null");
  if (dom->owner != ctx) return bad(ctx, "the domain belongs to another context");
  ntt::schedule S;
  const int cap = ntt_cap(flags);
  if (!cap || !ntt::make_schedule(dom->log_n, cap, &S)) return bad(ctx, "flags: 0 or ECSIMD_NTT_MAX_RADIX_LOG(1 .. 9)");
  if (batch == 0) return ECSIMD_HIP_OK;
  if (batch > (NTT_MAX_ELEMENTS >> dom->log_n)) return bad(ctx, "batch too large");
  if (!in || !out) return bad(ctx, "in or out is null");
  if (!aligned16(in) || !aligned16(out)) return bad(ctx, "in or out is not 16-byte aligned");
  const size_t bytes = (batch << dom->log_n) * 32;
  if (in != out && ranges_overlap(in, out, bytes)) return bad(ctx, "in and out overlap without being equal");
  hipError_t e = hipSetDevice(ctx->device);
  if (e != hipSuccess) return fail(ctx, e, "hipSetDevice");
  if (S.passes > 1) {
    int rc = ensure_workspace(ctx, bytes);
    if (rc != ECSIMD_HIP_OK) return rc;
    if (ranges_overlap(ctx->workspace, in, bytes) || ranges_overlap(ctx->workspace, out, bytes)) return bad(ctx, "in or out lies in the context's workspace");
  }
  const ntt::u4* src = reinterpret_cast<const ntt::u4*>(in);
  for (int i = 0; i < S.passes; ++i) {
    ntt::pass_args A;
    A.G = ntt::make_geom(dom->log_n, S, i, batch, inverse, dom->coset);
    A.tw = dom->tw[inverse];
    A.src = src;
    A.dst = reinterpret_cast<ntt::u4*>(ntt::pass_writes_workspace(i, S.passes) ? ctx->workspace : out);
    launch::ntt_pass(ctx->stream, dom->M, A);
    src = A.dst;
  }
  e = hipGetLastError();
  return e == hipSuccess ? ECSIMD_HIP_OK : fail(ctx, e, "ntt pass launch");
}
}  // namespace

extern "C" {
int ecsimd_ntt_plan(int log_n, size_t batch, int flags, ecsimd_ntt_plan_t* out) {
  ntt::schedule S;
  const int cap = ntt_cap(flags);
  if (!out || !cap || !ntt::make_schedule(log_n, cap, &S) || batch == 0 || batch > (NTT_MAX_ELEMENTS >> log_n)) return ECSIMD_HIP_ERR_BAD_ARG;
  static_assert(ECSIMD_NTT_MAX_PASSES == ntt::MAX_PASSES && ECSIMD_NTT_MAX_LOG_N == ntt::MAX_LOG_N && ECSIMD_NTT_DEFAULT_RADIX_LOG == ntt::DEFAULT_RADIX_LOG, "ecsimd_ntt.h restates ntt.cuh");
  memset(out, 0, sizeof *out);
  out->passes = out->launches = S.passes;
  for (int i = 0; i < ntt::MAX_PASSES; ++i) out->log_radix[i] = S.log_radix[i];
  out->lanes = ntt::LANES;
  out->lds_bytes = ntt::LDS_BYTES;
  out->workspace_bytes = S.passes > 1 ? (batch << log_n) * 32 : 0;
  return ECSIMD_HIP_OK;
}

int ecsimd_ntt_field_info(int field, int* two_adicity, uint64_t root[4]) {
  gmod M;
  if (!ntt_field(field, &M)) return ECSIMD_HIP_ERR_BAD_ARG;
  const pfield F = pfield_of(M);
  const field_facts K = facts_of(M);
  if (two_adicity) *two_adicity = K.s;
  if (root) { const u256 r = u_of(from_mgry(F, default_root_mgry(F, K))); memcpy(root, r.l, 32); }
  return ECSIMD_HIP_OK;
}

int ecsimd_ntt_bls12_381_fr(int* field, uint64_t root[4]) {
  if (!field) return ECSIMD_HIP_ERR_BAD_ARG;
  int rc = ecsimd_hip_register_modulus(FR_LIMBS, ECSIMD_HIP_MODULUS_PRIME, field);
  if (rc != ECSIMD_HIP_OK || !root) return rc;
  gmod M;
  if (!ntt_field(*field, &M)) return ECSIMD_HIP_ERR_BAD_ARG;
  const pfield F = pfield_of(M);
  const field_facts K = facts_of(M);
  pel seven = K.one;
  for (int i = 0; i < 6; ++i) seven = F.add(seven, K.one);
  const u256 r = u_of(from_mgry(F, p_pow(F, K.one, seven, u_shr(K.pm1, K.s))));
  memcpy(root, r.l, 32);
  return ECSIMD_HIP_OK;
}

int ecsimd_ntt_domain_create(ecsimd_hip_ctx* ctx, int field, int log_n, const uint64_t root[4], const uint64_t shift[4], ecsimd_ntt_domain** dom) {
  REQUIRE_CTX();
  if (!dom) return bad(ctx, "dom is null");
  *dom = nullptr;
  REFUSE_IN_CAPTURE("ntt_domain_create allocates, uploads its tables and waits for the copy");
  gmod M;
  if (!ntt_field(field, &M)) return bad(ctx, "field: not a modulus registered as prime");
  const pfield F = pfield_of(M);
  const field_facts K = facts_of(M);
  if (log_n < 1 || log_n > ntt::MAX_LOG_N || log_n > K.s) return bad(ctx, "log_n: 1 .. min(the field's two-adicity, 24)");
  u256 p; words_to_limbs(M.p, p.l);
  pel rt;
  if (root) {
    if (u_geq(u_from(root), p)) return bad(ctx, "root is not below p");
    rt = to_mgry(F, pel_of(u_from(root)));
    pel t = rt;
    for (int i = 0; i + 1 < K.s; ++i) t = F.mul(t, t);
    if (!pel_eq(t, K.minus_one)) return bad(ctx, "root is not a primitive 2^s-th root of unity: root^(2^(s-1)) != -1");
  } else rt = default_root_mgry(F, K);
  pel g = K.one;
  if (shift) {
    if (u_is_zero(u_from(shift)) || u_geq(u_from(shift), p)) return bad(ctx, "shift: 0 < shift < p");
    g = to_mgry(F, pel_of(u_from(shift)));
  }
  const int coset = !pel_eq(g, K.one);
  pel w = rt;
  for (int i = 0; i < K.s - log_n; ++i) w = F.mul(w, w);                    // w = root^(2^(s - log_n))
  u256 pm2; { const u256 one = {{1, 0, 0, 0}}; (void)u_sub(pm2, K.pm1, one); }
  pel nm = K.one;
  for (int i = 0; i < log_n; ++i) nm = F.add(nm, nm);                       // n
  const pel ninv = p_pow(F, K.one, nm, pm2);
  const size_t n = (size_t)1 << log_n, lo_n = n < (size_t)ntt::SPLIT ? n : (size_t)ntt::SPLIT, hi_n = n > (size_t)ntt::SPLIT ? n >> ntt::SPLIT_LOG : 1;
  const int log_rt = log_n < ntt::DEFAULT_RADIX_LOG ? log_n : ntt::DEFAULT_RADIX_LOG;
  const size_t stage_n = (size_t)1 << (log_rt - 1), per_dir = stage_n + 2 * lo_n + 2 * hi_n;
  ecsimd_ntt_domain* D = nullptr;
  std::vector<pel> host;
  try { host.reserve(2 * per_dir); D = new ecsimd_ntt_domain; }
  catch (...) { return bad(ctx, "ntt domain: out of host memory"); }
  auto powers = [&](const pel& base, size_t count, const pel& first) { pel t = first; for (size_t i = 0; i < count; ++i) { host.push_back(t); t = F.mul(t, base); } };
  auto pow2k = [&](pel v, int k) { for (int i = 0; i < k; ++i) v = F.mul(v, v); return v; };
  size_t off[2][5];
  for (int dir = 0; dir < 2; ++dir) {
    const pel wd = dir ? p_pow(F, K.one, w, pm2) : w, gd = dir ? p_pow(F, K.one, g, pm2) : g;
    off[dir][0] = host.size(); powers(pow2k(wd, log_n - log_rt), stage_n, K.one);
    off[dir][1] = host.size(); powers(wd, lo_n, K.one);
    off[dir][2] = host.size(); powers(pow2k(wd, ntt::SPLIT_LOG), hi_n, K.one);
    off[dir][3] = host.size(); powers(gd, lo_n, K.one);
    // forward: g^(SPLIT i) R^2 (Montgomery form twice over); inverse: n^-1 g^(-SPLIT i), classical
    off[dir][4] = host.size(); powers(pow2k(gd, ntt::SPLIT_LOG), hi_n, dir ? from_mgry(F, ninv) : to_mgry(F, K.one));
  }
  D->owner = ctx; D->M = M; D->log_n = log_n; D->coset = coset; D->block = nullptr;
  (void)hipSetDevice(ctx->device);
  hipError_t e = hipMalloc(&D->block, host.size() * sizeof(pel));
  if (e == hipSuccess) e = hipMemcpyAsync(D->block, host.data(), host.size() * sizeof(pel), hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);               // `host` must outlive the copy
  if (e != hipSuccess) { (void)hipFree(D->block); delete D; return fail(ctx, e, "ntt domain tables"); }
  for (int dir = 0; dir < 2; ++dir) {
    const ntt::u4* b = D->block;
    D->tw[dir] = ntt::tables{b + 2 * off[dir][0], b + 2 * off[dir][1], b + 2 * off[dir][2], b + 2 * off[dir][3], b + 2 * off[dir][4]};
  }
  *dom = D;
  return ECSIMD_HIP_OK;
}

int ecsimd_ntt_domain_destroy(ecsimd_hip_ctx* ctx, ecsimd_ntt_domain* dom) {
  REQUIRE_CTX();
  if (!dom) return ECSIMD_HIP_OK;
  if (dom->owner != ctx) return bad(ctx, "the domain belongs to another context");
  REFUSE_IN_CAPTURE("ntt_domain_destroy releases device memory, which waits for the device");
  (void)hipSetDevice(ctx->device);
  hipError_t e = hipFree(dom->block);
  delete dom;
  return e == hipSuccess ? ECSIMD_HIP_OK : fail(ctx, e, "hipFree");
}

int ecsimd_ntt_forward(ecsimd_hip_ctx* ctx, const ecsimd_ntt_domain* dom, const uint64_t* in, uint64_t* out, size_t batch, int flags) {
  return ntt_transform(ctx, dom, in, out, batch, flags, 0);
}
int ecsimd_ntt_inverse(ecsimd_hip_ctx* ctx, const ecsimd_ntt_domain* dom, const uint64_t* in, uint64_t* out, size_t batch, int flags) {
  return ntt_transform(ctx, dom, in, out, batch, flags, 1);
}

int ecsimd_ntt_bitrev(ecsimd_hip_ctx* ctx, int log_n, const uint64_t* in, uint64_t* out, size_t batch) {
  REQUIRE_CTX();
  if (log_n < 1 || log_n > ntt::MAX_LOG_N) return bad(ctx, "log_n: 1 .. 24");
  if (batch == 0) return ECSIMD_HIP_OK;
  if (batch > (NTT_MAX_ELEMENTS >> log_n)) return bad(ctx, "batch too large");
  if (!in || !out) return bad(ctx, "in or out is null");
  if (!aligned16(in) || !aligned16(out)) return bad(ctx, "in or out is not 16-byte aligned");
  if (in != out && ranges_overlap(in, out, (batch << log_n) * 32)) return bad(ctx, "in and out overlap without being equal");
  hipError_t e = hipSetDevice(ctx->device);
  if (e != hipSuccess) return fail(ctx, e, "hipSetDevice");
  launch::ntt_bitrev(ctx->stream, in, out, log_n, batch);
  e = hipGetLastError();
  return e == hipSuccess ? ECSIMD_HIP_OK : fail(ctx, e, "ntt bitrev launch");
}
}  // extern "C"
