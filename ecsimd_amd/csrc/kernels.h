// kernels.h -- host-side launchers, one per kernel family (defined in the k_*.hip files, which are
// compiled in parallel by the Makefile; the ladder alone takes ~1 min of hipcc time per curve).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace ecsimd_hip {
struct gmod;                 // gfield.cuh: a run-time modulus and what the field layer derives from it
struct gcurve;               // gcurve.cuh: a run-time curve (its field, a R, b R, the generator, the ladder loop's 29-bit constants)
struct g1_curve;             // tags: the two BLS12-381 groups as bls381_launch's instances (k_bls12_381.hip, k_bls12_381_g2.hip)
struct g2_curve;
namespace ntt { struct pass_args; }   // ntt.cuh: one pass of a number-theoretic transform (buffers, tables, geometry)
namespace launch {

constexpr int BLOCK = 256;   // one wave per SIMD of a CU; several workgroups resident per CU
inline dim3 grid_for(size_t n) { return dim3((unsigned)((n + BLOCK - 1) / BLOCK)); }

struct words8 { uint32_t w[8]; };   // a 256-bit kernel argument (exponent / shared scalar)

// k_bignum.hip (curve independent)
void add(hipStream_t, const uint64_t* a, const uint64_t* b, uint64_t* out, uint8_t* carry, size_t n);
void sub(hipStream_t, const uint64_t* a, const uint64_t* b, uint64_t* out, uint8_t* borrow, size_t n);
void sub_if_above(hipStream_t, const uint64_t* a, const uint64_t* p, uint64_t* out, size_t n);
void shift_left_one(hipStream_t, const uint64_t* a, uint64_t* out, uint8_t* carry, size_t n);
void mul(hipStream_t, const uint64_t* a, const uint64_t* b, uint64_t* out8, size_t n);
void square(hipStream_t, const uint64_t* a, uint64_t* out8, size_t n, bool ref_compat = false);   // ref_compat: mul.h:160-212 as written
void swap_if(hipStream_t, const uint8_t* mask, uint64_t* a, uint64_t* b, size_t n);
void if_else(hipStream_t, const uint8_t* mask, const uint64_t* a, const uint64_t* b, uint64_t* out, size_t n);
void patch_special(hipStream_t, const uint64_t* k, const uint64_t* special /* 3 scalars, 3 x, 3 y */, uint64_t* ox, uint64_t* oy, size_t n);   // oy may be null
void cmp_eq(hipStream_t, const uint64_t* a, const uint64_t* b, int limbs, uint8_t* flag, size_t n);
void mask_op(hipStream_t, int op, const uint8_t* a, const uint8_t* b, uint8_t* out, size_t n);     // 0 not, 1 and, 2 or, 3 equal
void mask_count(hipStream_t, const uint8_t* a, size_t n, unsigned long long* count);
void fill_random(hipStream_t, uint64_t* out, size_t n, uint64_t seed, uint64_t stream, uint64_t first, int clear_top);
void peak_mad32(hipStream_t, int blocks, uint32_t* sink, int iters, uint32_t seed);
constexpr int PEAK_MADS_PER_LANE_PER_ITER = 64;

// k_serial.hip (wire formats; HBM-bound)
void bytes_be(hipStream_t, const void* in, void* out, size_t n);
void mask_bit(hipStream_t, const uint64_t* a, int bit, uint8_t* flag, size_t n);
void wide4_to_lanes(hipStream_t, const void* wides, size_t record_bytes, size_t offset_bytes, uint64_t* out, size_t n);      // n = ELEMENTS (4 per wide)
void lanes_to_wide4(hipStream_t, const uint64_t* in, void* wides, size_t record_bytes, size_t offset_bytes, size_t n);
void sec1_encode(hipStream_t, int curve, const uint64_t* x, const uint64_t* y, uint8_t* out, size_t n, bool compressed);
void sec1_decode(hipStream_t, int curve, const uint8_t* in, uint64_t* x, uint64_t* y, uint8_t* ok, size_t n, bool compressed);
void on_curve(hipStream_t, int curve, const uint64_t* x, const uint64_t* y, uint8_t* ok, size_t n);                 // classical (x, y): x, y < p and on the curve
void clear_invalid(hipStream_t, const uint8_t* valid, uint64_t* rx, uint64_t* ry, uint8_t* finite, size_t n);      // (0, 0) / not finite where !valid

// k_field.hip
enum field_op { F_MOD_ADD, F_MOD_SUB, F_MGRY_MUL, F_MGRY_SQR, F_FROM_CLASSICAL, F_TO_CLASSICAL, F_INVERSE, F_OPPOSITE };
void field_binop(hipStream_t, int curve, field_op op, const uint64_t* a, const uint64_t* b, uint64_t* out, size_t n);
void field_unop(hipStream_t, int curve, field_op op, const uint64_t* a, uint64_t* out, size_t n);
void mod_shift_left(hipStream_t, int curve, const uint64_t* a, int count, uint64_t* out, size_t n);
void mod_mul(hipStream_t, int curve, const uint64_t* a, const uint64_t* b, uint64_t* out, size_t n);
void mgry_reduce(hipStream_t, int curve, const uint64_t* a8, uint64_t* out, size_t n);
void mgry_pow(hipStream_t, int curve, const uint64_t* a, const words8& e, uint64_t* out, size_t n);
void gfp_sqrt(hipStream_t, int curve, const uint64_t* a, uint64_t* out, uint8_t* ok, size_t n);

// k_gfield.hip: the same layer for a RUN-TIME modulus (any odd 256-bit value: the group orders, a caller's own prime); ref_square =
// the reference's square() as written.  F_INVERSE: division steps for a prime modulus, x^(p-2) bit by bit otherwise (gfp.h:42-44).
void gfield_binop(hipStream_t, const gmod&, field_op op, const uint64_t* a, const uint64_t* b, uint64_t* out, size_t n);
void gfield_unop(hipStream_t, const gmod&, field_op op, const uint64_t* a, uint64_t* out, size_t n, bool ref_square);
void gfield_mod_mul(hipStream_t, const gmod&, const uint64_t* a, const uint64_t* b, uint64_t* out, size_t n);
void gfield_shift_left(hipStream_t, const gmod&, const uint64_t* a, int count, uint64_t* out, size_t n);
void gfield_reduce(hipStream_t, const gmod&, const uint64_t* a8, uint64_t* out, size_t n);
void gfield_pow(hipStream_t, const gmod&, const uint64_t* a, const words8& e, uint64_t* out, size_t n, bool ref_square);
void gfield_sqrt(hipStream_t, const gmod&, const uint64_t* a, uint64_t* out, uint8_t* ok, size_t n, bool ref_square);
void gfield_inverse_batched(hipStream_t, const gmod&, const uint64_t* a, uint64_t* out, size_t n);   // prime modulus; out must not alias a
// ECDSA verification's arithmetic modulo the group order (gmod of n): valid = 1 <= r, s < n; u1 = e / s, u2 = r / s (0, 0 where invalid)
void ecdsa_scalars(hipStream_t, const gmod& order, const uint64_t* e, const uint64_t* r, const uint64_t* s, uint64_t* u1, uint64_t* u2, uint8_t* valid, size_t n);
// ECDSA signing's arithmetic modulo the group order: r = x mod n, s = (e + r d) / k; ok = the inputs are in range and r, s != 0 (secret d, k: selects only)
void ecdsa_sign_scalars(hipStream_t, const gmod& order, const uint64_t* e, const uint64_t* d, const uint64_t* k, const uint64_t* x, uint64_t* r, uint64_t* s, uint8_t* ok, size_t n);

// k_gcurve.hip / k_gladder.hip: the point layer and the ladder for a curve registered at RUN time (curve_group<Curve> for any Curve: curve.h:12-15).
// ref = the reference's square() as written; gc_scalar_mult flags: ECSIMD_HIP_BASE_MGRY | LADDER_RADIX32 | REF_SQUARE_COMPAT (Jacobian Montgomery out).
void gc_from_affine(hipStream_t, const gcurve&, const uint64_t* x, const uint64_t* y, uint64_t* jx, uint64_t* jy, uint64_t* jz, size_t n);
void gc_to_affine(hipStream_t, const gcurve&, const uint64_t* jx, const uint64_t* jy, const uint64_t* jz, uint64_t* x, uint64_t* y, size_t n, bool ref);
void gc_to_affine_batched(hipStream_t, const gcurve&, const uint64_t* jx, const uint64_t* jy, const uint64_t* jz, uint64_t* x, uint64_t* y, size_t n);   // x / y must not alias the inputs
void gc_compute_y(hipStream_t, const gcurve&, const uint64_t* x, uint64_t* y, uint8_t* ok, size_t n, bool ref);
void gc_on_curve(hipStream_t, const gcurve&, const uint64_t* x, const uint64_t* y, uint8_t* ok, size_t n);
void gc_dblu(hipStream_t, const gcurve&, uint64_t* px, uint64_t* py, uint64_t* pz, uint64_t* rx, uint64_t* ry, uint64_t* rz, size_t n, bool ref);
void gc_zaddu(hipStream_t, const gcurve&, uint64_t* px, uint64_t* py, uint64_t* pz, const uint64_t* qx, const uint64_t* qy, uint64_t* rx, uint64_t* ry, uint64_t* rz, size_t n, bool ref);
void gc_zdau(hipStream_t, const gcurve&, const uint64_t* px, const uint64_t* py, const uint64_t* pz, uint64_t* qx, uint64_t* qy, uint64_t* qz, uint64_t* rx, uint64_t* ry, uint64_t* rz, size_t n, bool ref);
void gc_add_z2_1(hipStream_t, const gcurve&, const uint64_t* ax, const uint64_t* ay, const uint64_t* az, const uint64_t* bx, const uint64_t* by, uint64_t* rx, uint64_t* ry, uint64_t* rz, size_t n, bool ref);
void gc_trplu(hipStream_t, const gcurve&, uint64_t* px, uint64_t* py, uint64_t* pz, uint64_t* rx, uint64_t* ry, uint64_t* rz, size_t n, bool ref);
void gc_scalar_mult(hipStream_t, const gcurve&, const uint64_t* k, int k_stride, const uint64_t* x, const uint64_t* y, uint64_t* ox, uint64_t* oy, uint64_t* oz, size_t n, int flags);
// k_gcomb.hip: k G on a registered curve from a 4-bit odd-digit table of multiples of its generator in LDS (64 windows x 8 entries x 64 B + k* G + k*)
constexpr int GCOMB_WINDOWS = 64, GCOMB_ENTRIES = 8;
void gc_pack_table(hipStream_t, const gcurve& G, const uint64_t* tx, const uint64_t* ty, uint32_t* table, int entries);
void gc_base_windowed(hipStream_t, const gcurve& G, const words8& order, const uint64_t* k, const uint32_t* table, uint64_t* ox, uint64_t* oy, uint64_t* oz, size_t n, bool constant_time);
// ... and from signed 7-bit windows with odd digits (37 windows x 64 entries, 148 KiB of LDS, summed from the bottom: ALG_WINDOWED_SIGNED; public scalars)
// ... and the constant-time 5-bit comb (52 windows x 16 entries, 53 KB of LDS, every entry of a window read: ALG_WINDOWED | ALG_CONSTANT_TIME, k G of ecdsa_sign)
constexpr int GCOMB7_BITS = 7, GCOMB7_WINDOWS = 37, GCOMB7_ENTRIES = 64, GCOMB5_WINDOWS = 52, GCOMB5_ENTRIES = 16, GCOMB20_WINDOWS = 13, GCOMB20_ENTRIES = 1 << 19;   // (20 bits: 436 MB in device memory, ALG_WINDOWED_BIG)
void gc_base_windowed_s(hipStream_t, const gcurve& G, const words8& order, int bits, const uint64_t* k, const uint32_t* table, uint64_t* ox, uint64_t* oy, uint64_t* oz, size_t n);
// k_gvarwin.hip: k P on a registered curve with per-lane window tables (the eight odd multiples of P over one Z, the loop on the isomorphic curve; affine
// classical out, oy may be null).  scratch: gc_varwin_scratch_bytes(n) bytes, 32-byte aligned; k_stride, x, y as for gc_scalar_mult; flags: ECSIMD_HIP_BASE_MGRY.
inline size_t gc_varwin_scratch_bytes(size_t n) { return n * (8 * 64 + 32 + 3 * 32); }
void gc_varwin_scalar_mult(hipStream_t, const gcurve& G, const words8& order, const uint64_t* k, int k_stride, const uint64_t* x, const uint64_t* y, int flags,
                           uint64_t* scratch, uint64_t* ox, uint64_t* oy, size_t n);
// ... and what ECDSA on a registered curve needs on top (public-data affine addition, the acceptance test, the ladder's three degenerate scalars worked around)
void gc_affine_add_batched(hipStream_t, const gcurve&, const uint64_t* ax, const uint64_t* ay, const uint64_t* bx, const uint64_t* by, uint64_t* rx, uint64_t* ry, uint8_t* finite, size_t n);
void gc_x_mod_n_equals(hipStream_t, const gmod& order, const uint64_t* x, const uint8_t* finite, const uint64_t* r, uint8_t* ok, size_t n);
void gc_ladder_safe_scalars(hipStream_t, const gmod& order, const uint64_t* u, uint64_t* adj, uint8_t* neg, size_t n);
void gc_negate_where(hipStream_t, const gcurve&, const uint8_t* neg, uint64_t* y, size_t n);
void gc_sec1_decode(hipStream_t, const gcurve&, const uint8_t* in, uint64_t* x, uint64_t* y, uint8_t* ok, size_t n, bool compressed);
void gc_zdau_repeat(hipStream_t, const gcurve&, const uint64_t* px, const uint64_t* py, const uint64_t* pz, const uint64_t* qx, const uint64_t* qy,
                    uint64_t* rx, uint64_t* ry, uint64_t* sx, uint64_t* sy, uint64_t* oz, size_t n, int iters, uint64_t swap_bits, int radix);

// k_recover.hip: ECDSA public-key recovery's front end (public data) and the recovery id of a signature just made (secret data: selects only).
// recover_lift / gc_recover_lift: x = r + (v >> 1) n, y = the root of x^3 + a x + b with the parity of v; valid = v <= 3, x < p, the root exists (R = G where not).
// ecdsa_recover_scalars: valid &= 1 <= r, s < n; u1 = -e / r, u2 = s / r modulo the order (0, 0 where not valid); one shared inversion per up to 128 elements.
void recover_lift(hipStream_t, int curve, const words8& order, const uint64_t* r, const uint8_t* v, uint64_t* x, uint64_t* y, uint8_t* valid, size_t n);
void gc_recover_lift(hipStream_t, const gcurve&, const words8& order, const uint64_t* r, const uint8_t* v, uint64_t* x, uint64_t* y, uint8_t* valid, size_t n);
void ecdsa_recover_scalars(hipStream_t, const gmod& order, const uint64_t* e, const uint64_t* r, const uint64_t* s, uint64_t* u1, uint64_t* u2, uint8_t* valid, size_t n);
// v = parity(y) | (x >= n ? 2 : 0), 0 where !ok; low_s: s > n / 2 becomes n - s and flips bit 0 of v.  (x, y) = the affine k G.
void sign_recovery_id(hipStream_t, const words8& order, const uint64_t* x, const uint64_t* y, uint64_t* s, const uint8_t* ok, uint8_t* v, size_t n, bool low_s);

// k_sha256.hip: SHA-256 of n equal-length messages (message i at msg + i * stride_bytes; e = the digests as 256-bit integers), and the RFC 6979 nonce
// (HMAC-SHA-256, qlen = 256): k = the nonce of (e, d), ok = 0 and k = 0 where d is not in [1, n - 1] or `cap` candidates were all out of range.  state: 96 B per
// element (K as its two HMAC midstates, V), retry: one byte per element -- the one declassified bit, "the last candidate was rejected".  Secret: d, k, state.
void sha256(hipStream_t, const uint8_t* msg, size_t msg_bytes, size_t stride_bytes, uint64_t* e, size_t n);
void rfc6979_nonce(hipStream_t, const words8& order, const uint64_t* e, const uint64_t* d, uint64_t* k, void* state, uint8_t* retry, uint8_t* ok, size_t n, unsigned cap);

// k_keccak.hip: Keccak-256 (the original padding: 0x01 ... 0x80, rate 136) of n messages, one per lane, and what Ethereum makes of it.  PUBLIC data only.
// keccak256: message i at msg + i * stride_bytes, lens[i] bytes of it where lens != NULL (lens[i] <= stride_bytes), else msg_bytes; e = the digests as 256-bit
// integers (sha256's convention).  eth_address: the low 20 bytes of Keccak-256(be32(qx) || be32(qy)) at addr + 20 i (addr 4-byte aligned), 20 zero bytes where
// ok != NULL and ok[i] = 0.  eth_recovery_id: v in {0, 1, 27, 28} -> 0 / 1, anything else (and, with low_s, s > half = n / 2) -> 0xff, which recover_lift refuses.
void keccak256(hipStream_t, const uint8_t* msg, size_t msg_bytes, size_t stride_bytes, const uint32_t* lens, uint64_t* e, size_t n);
void eth_address(hipStream_t, const uint64_t* qx, const uint64_t* qy, const uint8_t* ok, uint8_t* addr, size_t n);
void eth_recovery_id(hipStream_t, const words8& half, const uint8_t* v, const uint64_t* s, uint8_t* out, size_t n, bool low_s);

// k_schnorr.hip: BIP-340 on secp256k1.  Verification (public data): schnorr_verify_front writes u1 = s, u2 = n - e mod n with e = the challenge hash of
// (r, px, message), (x, y) = the even-y lift of px (G where there is none) and valid = lift && r < p && s < n (u1 = u2 = 0 where not); schnorr_accept:
// ok = finite && x == r && y even for the sum (x, y).  Signing (SECRET d, aux, k0 and both affine products: selects only): schnorr_nonce writes k0 from
// (d, aux or NULL, the affine d G, message), 0 where d is not in [1, n - 1]; schnorr_finish writes r, s, px (may be NULL) and ok from (d, k0, d G, k0 G, message).
void schnorr_verify_front(hipStream_t, const words8& order, const uint64_t* px, const uint64_t* r, const uint64_t* s, const uint8_t* msg, size_t msg_bytes, size_t stride_bytes,
                          uint64_t* u1, uint64_t* u2, uint64_t* x, uint64_t* y, uint8_t* valid, size_t n);
void schnorr_accept(hipStream_t, const uint64_t* x, const uint64_t* y, const uint8_t* finite, const uint64_t* r, uint8_t* ok, size_t n);
void schnorr_nonce(hipStream_t, const words8& order, const uint64_t* d, const uint64_t* aux, const uint64_t* px, const uint64_t* py, const uint8_t* msg, size_t msg_bytes,
                   size_t stride_bytes, uint64_t* k0, size_t n);
void schnorr_finish(hipStream_t, const gmod& order, const uint64_t* d, const uint64_t* k0, const uint64_t* xP, const uint64_t* yP, const uint64_t* xR, const uint64_t* yR,
                    const uint8_t* msg, size_t msg_bytes, size_t stride_bytes, uint64_t* px, uint64_t* r, uint64_t* s, uint8_t* ok, size_t n);

// k_btc.hip: what Bitcoin makes of SHA-256 and secp256k1.  The hashes (PUBLIC data; messages as for sha256): ripemd160 and hash160 = RIPEMD160(SHA256(m)) write
// 20 bytes per lane at out20 + 20 i (4-byte aligned), sha256d = SHA256(SHA256(m)) writes e as sha256 does, btc_pubkey_hash = hash160 of the SEC1 encoding of
// (qx, qy), built in registers.  The Taproot tweaks: tweak_front writes (x, y) = the even-y lift of px (G where the lane is refused), tt = t (mode 0), or
// int(H_TapTweak(px)) / int(H_TapTweak(px || merkle)) (modes 1 / 2), 0 where refused, and valid = lift && t < n; tweak_add: J += (x, y), complete (J Jacobian in
// the fast domain, Z = 0 is infinity); tweak_accept: ok = valid && Z != 0, qx = ax and parity = ay & 1 under it.  taproot_seckey (SECRET d, the affine d G,
// d_out: selects only): d_out = (d or n - d by the parity of y(d G)) + t mod n, px (may be NULL) = x(d G), all 0 where d is not in [1, n - 1], t >= n or the sum is 0.
enum tweak_mode { TWEAK_GIVEN = 0, TWEAK_KEY_PATH = 1, TWEAK_MERKLE_ROOT = 2 };
void ripemd160(hipStream_t, const uint8_t* msg, size_t msg_bytes, size_t stride_bytes, uint8_t* out20, size_t n);
void hash160(hipStream_t, const uint8_t* msg, size_t msg_bytes, size_t stride_bytes, uint8_t* out20, size_t n);
void sha256d(hipStream_t, const uint8_t* msg, size_t msg_bytes, size_t stride_bytes, uint64_t* e, size_t n);
void btc_pubkey_hash(hipStream_t, const uint64_t* qx, const uint64_t* qy, uint8_t* out20, size_t n, bool compressed);
void tweak_front(hipStream_t, const words8& order, int mode, const uint64_t* px, const uint64_t* t_or_merkle, uint64_t* x, uint64_t* y, uint64_t* tt, uint8_t* valid, size_t n);
void tweak_add(hipStream_t, uint64_t* jx, uint64_t* jy, uint64_t* jz, const uint64_t* x, const uint64_t* y, size_t n);
void tweak_accept(hipStream_t, const uint64_t* ax, const uint64_t* ay, const uint64_t* jz, const uint8_t* valid, uint64_t* qx, uint8_t* parity, uint8_t* ok, size_t n);
void taproot_seckey(hipStream_t, const gmod& order, const uint64_t* d, const uint64_t* merkle, const uint64_t* xP, const uint64_t* yP, uint64_t* d_out, uint64_t* px,
                    uint8_t* ok, size_t n);

// k_btc_tree.hip (PUBLIC data).  *_lens: the hashes above with lens[i] bytes of message i (lens != NULL, n x u32; a value above stride_bytes is read as
// stride_bytes); no byte at or behind a lane's message is loaded.  merkle_level: one level of `trees` Merkle trees -- off_in / off_out are the trees + 1 node
// offsets of the level read and the level written (device memory), n = off_out[trees] parents; mutated (may be NULL) gets a 1 per tree with a real pair of equal
// nodes.  tapleaf_hash: e = H_TapLeaf(version || compact_size(len) || script), scripts addressed as messages (lens may be NULL: script_bytes each), version
// n x u8 or NULL for version_all.  taproot_merkle_path: root = the TapBranch walk from leaf over depth[i] (NULL: depth_all) nodes of 32 bytes at
// path + i * path_stride_bytes; ok = 0 and root = 0 where the depth is above 128.
void sha256_lens(hipStream_t, const uint8_t* msg, size_t stride_bytes, const uint32_t* lens, uint64_t* e, size_t n);
void sha256d_lens(hipStream_t, const uint8_t* msg, size_t stride_bytes, const uint32_t* lens, uint64_t* e, size_t n);
void hash160_lens(hipStream_t, const uint8_t* msg, size_t stride_bytes, const uint32_t* lens, uint8_t* out20, size_t n);
void ripemd160_lens(hipStream_t, const uint8_t* msg, size_t stride_bytes, const uint32_t* lens, uint8_t* out20, size_t n);
void merkle_level(hipStream_t, const uint64_t* in, const uint64_t* off_in, const uint64_t* off_out, size_t trees, uint64_t* out, uint8_t* mutated, size_t n);
void tapleaf_hash(hipStream_t, const uint8_t* script, size_t script_bytes, size_t stride_bytes, const uint32_t* lens, const uint8_t* version, uint32_t version_all, uint64_t* e,
                  size_t n);
void taproot_merkle_path(hipStream_t, const uint64_t* leaf, const uint8_t* path, size_t path_stride_bytes, const uint8_t* depth, uint32_t depth_all, uint64_t* root, uint8_t* ok,
                         size_t n);

// k_sha512.hip: SHA-512 and HMAC-SHA-512 of n equal-length messages (PUBLIC data; messages as for sha256); 64 digest bytes per lane at out64 + 64 i (16-byte
// aligned).  hmac_sha512: lane i's key at key + i * key_stride_bytes (0: one key for the call), zero-padded to a block or, beyond 128 bytes, hashed first.
void sha512(hipStream_t, const uint8_t* msg, size_t msg_bytes, size_t stride_bytes, uint8_t* out64, size_t n);
void hmac_sha512(hipStream_t, const uint8_t* key, size_t key_bytes, size_t key_stride_bytes, const uint8_t* msg, size_t msg_bytes, size_t stride_bytes, uint8_t* out64, size_t n);

// k_bip32.hip: BIP-32 on secp256k1.  index == NULL: every lane uses index_all.  bip32_master (SECRET seed, k, c: selects only): (k, c) = the halves of
// HMAC-SHA512("Bitcoin seed", seed), seed_bytes in [16, 64]; zeros and ok = 0 where k = 0 or k >= n.  bip32_ckd_priv (SECRET k_par, c_par, the affine k_par G,
// k_child, c_child: selects only): CKDpriv; (xP, yP) = the affine k_par G, or both NULL: the kernel without point arrays, which refuses every lane whose index
// is not hardened.  bip32_ckd_pub_front (PUBLIC): t = IL, c_child = IR, (x, y) = K, valid = index < 2^31 && K on the curve && IL < n (t = 0, c_child = 0 and
// K = G where not); bip32_ckd_pub_accept: ok = valid && Z != 0, (cx, cy) = (ax, ay) under it, c_child zeroed where not.
void bip32_master(hipStream_t, const words8& order, const uint8_t* seed, size_t seed_bytes, size_t stride_bytes, uint64_t* k, uint64_t* c, uint8_t* ok, size_t n);
void bip32_ckd_priv(hipStream_t, const gmod& order, const uint64_t* k_par, const uint64_t* c_par, const uint32_t* index, uint32_t index_all, const uint64_t* xP, const uint64_t* yP,
                    uint64_t* k_child, uint64_t* c_child, uint8_t* ok, size_t n);
void bip32_ckd_pub_front(hipStream_t, const words8& order, const uint64_t* qx, const uint64_t* qy, const uint64_t* c_par, const uint32_t* index, uint32_t index_all, uint64_t* x,
                         uint64_t* y, uint64_t* t, uint64_t* c_child, uint8_t* valid, size_t n);
void bip32_ckd_pub_accept(hipStream_t, const uint64_t* ax, const uint64_t* ay, const uint64_t* jz, const uint8_t* valid, uint64_t* cx, uint64_t* cy, uint64_t* c_child, uint8_t* ok,
                          size_t n);

// k_pbkdf2.hip: PBKDF2-HMAC-SHA-512, one (password, salt) pair per lane and `blocks` 64-byte output blocks block_first .. block_first + blocks - 1 (the grid's y) of
// each.  SECRET contents, PUBLIC lengths: pw / salt as hmac_sha512's key (salt_stride_bytes == 0: one salt for the call), *_lens as keccak256's, any alignment.
// pre: pre_bytes (0 or 8) bytes that stand in front of every salt (big-endian in the word).  first: the set-up and U_1 run (otherwise the n * blocks units of 256 B
// at `state` are read); then `loops` times U = HMAC(P, U), T ^= U; last: T goes to out + i * out_stride_bytes + 64 block, dk_bytes in all (otherwise `state` is written).
void pbkdf2_hmac_sha512(hipStream_t, bool first, bool last, const uint8_t* pw, size_t pw_bytes, size_t pw_stride_bytes, const uint32_t* pw_lens, const uint8_t* salt,
                        size_t salt_bytes, size_t salt_stride_bytes, const uint32_t* salt_lens, uint64_t pre, unsigned pre_bytes, unsigned block_first, unsigned blocks,
                        unsigned loops, void* state, uint8_t* out, size_t dk_bytes, size_t out_stride_bytes, size_t n);

// k_fe29_raw.hip: one function of fe29.cuh on raw 9-limb operands (the diagnostic entry ecsimd_hip_fe29_raw)
enum fe29_raw_op { RAW_ZDAU = 0, RAW_MADD = 1, RAW_JDBL = 2, RAW_DBL_ADD = 3, RAW_MADDV = 4, RAW_PDBL = 5, RAW_PADD = 6, RAW_MUL = 7, RAW_SQR = 8, RAW_GJDBL = 9, RAW_ZADDU = 10 };
constexpr int fe29_raw_inputs(int op) { return op == RAW_ZDAU ? 6 : op == RAW_MUL ? 2 : op == RAW_SQR ? 1 : (op == RAW_JDBL || op == RAW_PDBL) ? 3 : op == RAW_GJDBL ? 4 : 5; }
constexpr int fe29_raw_outputs(int op) { return (op == RAW_ZDAU || op == RAW_ZADDU) ? 6 : (op == RAW_MUL || op == RAW_SQR) ? 1 : op == RAW_GJDBL ? 4 : 3; }
bool fe29_raw(hipStream_t, int curve, const gcurve* G, int op, const int32_t* in, int32_t* out, size_t n, uint32_t swap);

// k_ed25519.hip: Ed25519 (RFC 8032, pure).  L = the group order's gmod.  Keys, signatures and seeds are BYTES (32 / 64 / 32 per lane, any alignment: word
// accesses where the base is a multiple of 4); messages as keccak256's (lens may be NULL).  SECRET (selects only): ed25519_secret_front writes a = the clamped
// half of SHA-512(seed), reduced modulo L, and with sign = true r = SHA-512(prefix || M) mod L; ed25519_base_ct the 32-byte encodings of [k]B for n scalars below
// L; ed25519_sign_finish R || s with s = r + SHA-512(R || A || M) a mod L, and A at pk (may be NULL).  PUBLIC: ed25519_verify_front writes valid = s < L && A
// decodes (&& no small-order A or R), s, h = SHA-512(R || A || M) mod L and the lanes' tables of 1 .. 8 times -A (ed25519_table_bytes(n) bytes, 16-byte aligned);
// ed25519_verify_loop ok = valid && encode([s]B + [h](-A)) == R.  ed25519_raw: one function of the layers on 32-byte records (ED_RAW_DOUBLE_MULT needs the table).
enum ed25519_raw_op { ED_RAW_FE_MUL = 0, ED_RAW_FE_SQR = 1, ED_RAW_FE_ADD = 2, ED_RAW_FE_SUB = 3, ED_RAW_FE_NEG = 4, ED_RAW_FE_INVERT = 5, ED_RAW_FE_CANON = 6, ED_RAW_SQRT_RATIO = 7,
                      ED_RAW_DECODE_ENCODE = 8, ED_RAW_POINT_ADD = 9, ED_RAW_POINT_DBL = 10, ED_RAW_SC_REDUCE = 11, ED_RAW_BASE_MULT = 12, ED_RAW_DOUBLE_MULT = 13 };
constexpr int ed_raw_inputs(int op) { return op == ED_RAW_DOUBLE_MULT ? 3 : (op == ED_RAW_FE_MUL || op == ED_RAW_FE_ADD || op == ED_RAW_FE_SUB || op == ED_RAW_SQRT_RATIO || op == ED_RAW_POINT_ADD || op == ED_RAW_SC_REDUCE) ? 2 : 1; }
constexpr int ed_raw_outputs(int op) { return (op == ED_RAW_SQRT_RATIO || op == ED_RAW_DECODE_ENCODE || op == ED_RAW_POINT_ADD || op == ED_RAW_POINT_DBL || op == ED_RAW_DOUBLE_MULT) ? 2 : 1; }
inline size_t ed25519_table_bytes(size_t n) { return n * 8 * 128; }
void ed25519_secret_front(hipStream_t, const gmod& L, const uint8_t* seed, const uint8_t* msg, size_t msg_bytes, size_t stride_bytes, const uint32_t* lens, bool sign,
                          uint64_t* a, uint64_t* r, size_t n);
void ed25519_base_ct(hipStream_t, const uint64_t* k, uint8_t* out32, size_t n);
void ed25519_sign_finish(hipStream_t, const gmod& L, const uint64_t* a, const uint64_t* r, const uint8_t* encA, const uint8_t* encR, const uint8_t* msg, size_t msg_bytes,
                         size_t stride_bytes, const uint32_t* lens, uint8_t* sig, uint8_t* pk, size_t n);
void ed25519_verify_front(hipStream_t, const gmod& L, const uint8_t* pk, const uint8_t* sig, const uint8_t* msg, size_t msg_bytes, size_t stride_bytes, const uint32_t* lens,
                          bool reject_small_order, uint64_t* s, uint64_t* h, void* table, uint8_t* valid, size_t n);
void ed25519_verify_loop(hipStream_t, const uint64_t* s, const uint64_t* h, const void* table, const uint8_t* valid, const uint8_t* sig, uint8_t* ok, size_t n);
void ed25519_raw(hipStream_t, const gmod& L, int op, const uint8_t* in, uint8_t* out, void* table, size_t n);

// k_x25519.hip: X25519 (RFC 7748) and the Ed25519 key conversions.  Every array is n records of 32 little-endian bytes at any alignment; nothing uses a
// workspace.  SECRET (selects only): x25519 writes X25519(scalar, u) (clamped scalar, bit 255 of u dropped, 0 at infinity) and, where ok is given, ok = the
// output is not all zero; x25519_base X25519(scalar, 9) through the comb over the multiples of B (L = the group order's gmod); x25519_from_ed_seed the clamped
// low half of SHA-512(seed).  PUBLIC: x25519_from_ed_pk writes u = (1 + y) / (1 - y) and ok = the key decodes strictly and is no small-order encoding
// (u = 0 where not).  x25519_raw: one function of the layers on 32-byte records.
enum x25519_raw_op { X25519_RAW_FE_MUL_SMALL = 0, X25519_RAW_LADDER = 1, X25519_RAW_ED_TO_MONT = 2 };
constexpr int x25519_raw_inputs(int op) { return op == X25519_RAW_LADDER ? 2 : 1; }
constexpr int x25519_raw_outputs(int op) { return op == X25519_RAW_ED_TO_MONT ? 2 : 1; }
void x25519(hipStream_t, const uint8_t* scalar, const uint8_t* u, uint8_t* out, uint8_t* ok, size_t n);
void x25519_base(hipStream_t, const gmod& L, const uint8_t* scalar, uint8_t* out, size_t n);
void x25519_from_ed_pk(hipStream_t, const uint8_t* pk, uint8_t* u, uint8_t* ok, size_t n);
void x25519_from_ed_seed(hipStream_t, const uint8_t* seed, uint8_t* scalar, size_t n);
void x25519_raw(hipStream_t, int op, const uint8_t* in, uint8_t* out, size_t n);

// k_p384.hip: NIST P-384 (include/ecsimd_p384.h).  Integers are 48 big-endian bytes, keys and signatures 96, at any alignment; messages as keccak256's.
// table: the lanes' multiples 1 .. 8 of their point, p384_table_bytes(n) bytes, 4-byte aligned; kws: p384_nonce_bytes(n) bytes for k and its validity.
// SECRET (selects only): p384_pubkey writes d G and ok = 1 <= d < n; p384_ecdh x(d peer) and ok = 1 <= d < n && the peer decodes; p384_sign_nonce the first
// RFC 6979 candidate (HMAC-SHA-384) and valid = 1 <= d, k < n into kws; p384_sign_finish r || s from kws and ok.  PUBLIC: p384_sha384; p384_verify
// ok = 1 <= r, s < n && pub decodes && u1 G + u2 Q is not the identity && x(R) mod n = r.  p384_raw: one function of the layers on 48-byte records.
enum p384_raw_op { P384_RAW_FE_MUL = 0, P384_RAW_FE_SQR = 1, P384_RAW_FE_ADD = 2, P384_RAW_FE_SUB = 3, P384_RAW_FE_NEG = 4, P384_RAW_FE_INVERT = 5, P384_RAW_FE_CANON = 6,
                   P384_RAW_SC_MUL = 7, P384_RAW_SC_INVERT = 8, P384_RAW_DECODE_ENCODE = 9, P384_RAW_POINT_ADD = 10, P384_RAW_POINT_DBL = 11, P384_RAW_BASE_MULT = 12,
                   P384_RAW_VAR_MULT = 13, P384_RAW_DOUBLE_MULT = 14 };
constexpr int p384_raw_inputs(int op) {
  return op == P384_RAW_POINT_ADD ? 6 : op == P384_RAW_DOUBLE_MULT ? 4 : (op == P384_RAW_POINT_DBL || op == P384_RAW_VAR_MULT) ? 3
       : (op == P384_RAW_FE_MUL || op == P384_RAW_FE_ADD || op == P384_RAW_FE_SUB || op == P384_RAW_SC_MUL || op == P384_RAW_DECODE_ENCODE) ? 2 : 1;
}
constexpr int p384_raw_outputs(int op) { return op >= P384_RAW_DECODE_ENCODE ? 3 : 1; }
inline size_t p384_table_bytes(size_t n) { return n * 8 * 36 * 4; }
inline size_t p384_nonce_bytes(size_t n) { return n * 13 * 4; }
void p384_sha384(hipStream_t, const uint8_t* msg, size_t msg_bytes, size_t stride_bytes, const uint32_t* lens, uint8_t* digest, size_t n);
void p384_pubkey(hipStream_t, const uint8_t* d, uint8_t* pub, uint8_t* ok, size_t n);
void p384_ecdh(hipStream_t, const uint8_t* d, const uint8_t* peer, uint32_t* table, uint8_t* z, uint8_t* ok, size_t n);
void p384_sign_nonce(hipStream_t, const uint8_t* d, const uint8_t* digest, uint32_t* kws, size_t n);
void p384_sign_finish(hipStream_t, const uint8_t* d, const uint8_t* digest, const uint32_t* kws, uint8_t* sig, uint8_t* ok, size_t n);
void p384_verify(hipStream_t, const uint8_t* pub, const uint8_t* digest, const uint8_t* sig, uint32_t* table, uint8_t* ok, size_t n);
void p384_raw(hipStream_t, int op, const uint8_t* in, uint8_t* out, uint32_t* table, size_t n);

// k_point_<curve>.hip
void from_affine(hipStream_t, int curve, const uint64_t* x, const uint64_t* y, uint64_t* jx, uint64_t* jy, uint64_t* jz, size_t n);
void to_affine(hipStream_t, int curve, const uint64_t* jx, const uint64_t* jy, const uint64_t* jz, uint64_t* x, uint64_t* y, size_t n);
void compute_y(hipStream_t, int curve, const uint64_t* x, uint64_t* y, uint8_t* ok, size_t n);
void dblu(hipStream_t, int curve, uint64_t* px, uint64_t* py, uint64_t* pz, uint64_t* rx, uint64_t* ry, uint64_t* rz, size_t n);
void zaddu(hipStream_t, int curve, uint64_t* px, uint64_t* py, uint64_t* pz, const uint64_t* qx, const uint64_t* qy, uint64_t* rx, uint64_t* ry, uint64_t* rz, size_t n);
void zdau(hipStream_t, int curve, const uint64_t* px, const uint64_t* py, const uint64_t* pz, uint64_t* qx, uint64_t* qy, uint64_t* qz, uint64_t* rx, uint64_t* ry, uint64_t* rz, size_t n);
void add_z2_1(hipStream_t, int curve, const uint64_t* ax, const uint64_t* ay, const uint64_t* az, const uint64_t* bx, const uint64_t* by, uint64_t* rx, uint64_t* ry, uint64_t* rz, size_t n);
void trplu(hipStream_t, int curve, uint64_t* px, uint64_t* py, uint64_t* pz, uint64_t* rx, uint64_t* ry, uint64_t* rz, size_t n);

// k_ladder_<curve>.hip.  k_stride = 4 (u64 per element) for per-element scalars, 0 for one shared
// scalar (device memory either way).  x == nullptr selects the curve generator as base point.
// flags: ECSIMD_HIP_BASE_* | ECSIMD_HIP_OUT_*.
void scalar_mult(hipStream_t, int curve, const uint64_t* k, int k_stride, const uint64_t* x, const uint64_t* y,
                 uint64_t* ox, uint64_t* oy, uint64_t* oz, size_t n, int flags);
void zdau_repeat(hipStream_t, int curve, const uint64_t* px, const uint64_t* py, const uint64_t* pz, const uint64_t* qx, const uint64_t* qy,
                 uint64_t* rx, uint64_t* ry, uint64_t* sx, uint64_t* sy, uint64_t* oz, size_t n, int iters, uint64_t swap_bits, int radix);
// k_affine_<curve>.hip: simultaneous-inversion to_affine (x, y must not alias the inputs), the
// 4-bit-window table packer and the fixed-base windowed multiplication (Jacobian out, fast domain).
void to_affine_batched(hipStream_t, int curve, const uint64_t* jx, const uint64_t* jy, const uint64_t* jz, uint64_t* x, uint64_t* y, size_t n, bool in_fast_domain);
void inverse_batched(hipStream_t, int curve, const uint64_t* a, uint64_t* out, size_t n);     // out must not alias a
void x_mod_n_equals(hipStream_t, int curve, const uint64_t* x, const uint8_t* finite, const uint64_t* r, uint8_t* ok, size_t n);
void affine_add_batched(hipStream_t, int curve, const uint64_t* ax, const uint64_t* ay, const uint64_t* bx, const uint64_t* by, uint64_t* rx, uint64_t* ry, uint8_t* finite, size_t n);
void pack_table(hipStream_t, int curve, const uint64_t* tx, const uint64_t* ty, uint32_t* table);
void base_windowed(hipStream_t, int curve, const uint64_t* k, const uint32_t* table, uint64_t* ox, uint64_t* oy, uint64_t* oz, size_t n, bool constant_time);
// signed windows of wbits = 6 or 7 bits
void pack_table_signed(hipStream_t, int curve, int wbits, const uint64_t* tx, const uint64_t* ty, uint32_t* table);
void base_windowed_signed(hipStream_t, int curve, const uint64_t* k, const uint32_t* table, uint64_t* ox, uint64_t* oy, uint64_t* oz, size_t n, bool constant_time);

// k_varwin_<curve>.hip: variable-base multiplication with per-lane window tables of 8 multiples of P (affine out, classical).
// scratch: varwin_scratch_bytes(n) bytes, 32-byte aligned; k_stride, x, y as for scalar_mult (flags: ECSIMD_HIP_BASE_*).
void varwin_scalar_mult(hipStream_t, int curve, const uint64_t* k, int k_stride, const uint64_t* x, const uint64_t* y, int flags,
                        uint64_t* scratch, uint64_t* ox, uint64_t* oy, size_t n);
// complete mixed addition (A Jacobian, Z = 0 is infinity; B Montgomery-form affine, (0, 0) is infinity)
void add_mixed_complete(hipStream_t, int curve, const uint64_t* ax, const uint64_t* ay, const uint64_t* az, const uint64_t* bx, const uint64_t* by,
                        uint64_t* rx, uint64_t* ry, uint64_t* rz, size_t n);
inline size_t varwin_scratch_bytes(size_t n) { return n * (7 * 4 * 32 + 8 * 64); }

// signed BIG_WINDOW_BITS-bit windows over a table in device memory (20 bits: 13 windows x 524 288 entries x 64 B = 436 MB)
void pack_table_big(hipStream_t, int curve, const uint64_t* tx, const uint64_t* ty, uint32_t* table);
void base_windowed_big(hipStream_t, int curve, const uint64_t* k, const uint32_t* table, uint64_t* ox, uint64_t* oy, uint64_t* oz, size_t n);
#ifndef ECS_BIG_WINDOW_BITS
#define ECS_BIG_WINDOW_BITS 20   // measured on one MI355X, P-256 / secp256k1 M/s: 16 bits 904 / 883 (36 MB), 18 bits 995 / 965 (126 MB),
                                 // 20 bits 1 075 / 1 090 (436 MB, built in 0.23 s), 22 bits 1 124 / 1 146 (1.6 GB, 0.8 s)
#endif
constexpr int BIG_WINDOW_BITS = ECS_BIG_WINDOW_BITS;

// per-curve pieces (one translation unit each)
template <int C> struct point_launch {
  static void from_affine(hipStream_t, const uint64_t*, const uint64_t*, uint64_t*, uint64_t*, uint64_t*, size_t);
  static void to_affine(hipStream_t, const uint64_t*, const uint64_t*, const uint64_t*, uint64_t*, uint64_t*, size_t);
  static void compute_y(hipStream_t, const uint64_t*, uint64_t*, uint8_t*, size_t);
  static void dblu(hipStream_t, uint64_t*, uint64_t*, uint64_t*, uint64_t*, uint64_t*, uint64_t*, size_t);
  static void zaddu(hipStream_t, uint64_t*, uint64_t*, uint64_t*, const uint64_t*, const uint64_t*, uint64_t*, uint64_t*, uint64_t*, size_t);
  static void zdau(hipStream_t, const uint64_t*, const uint64_t*, const uint64_t*, uint64_t*, uint64_t*, uint64_t*, uint64_t*, uint64_t*, uint64_t*, size_t);
  static void add_z2_1(hipStream_t, const uint64_t*, const uint64_t*, const uint64_t*, const uint64_t*, const uint64_t*, uint64_t*, uint64_t*, uint64_t*, size_t);
  static void trplu(hipStream_t, uint64_t*, uint64_t*, uint64_t*, uint64_t*, uint64_t*, uint64_t*, size_t);
  static void scalar_mult(hipStream_t, const uint64_t*, int, const uint64_t*, const uint64_t*, uint64_t*, uint64_t*, uint64_t*, size_t, int);
  static void zdau_repeat(hipStream_t, const uint64_t* px, const uint64_t* py, const uint64_t* pz, const uint64_t* qx, const uint64_t* qy,
                          uint64_t* rx, uint64_t* ry, uint64_t* sx, uint64_t* sy, uint64_t* oz, size_t n, int iters, uint64_t swap_bits, int radix);
  // x(kP) only, by the ladder without Z (defined for P-256 only: needs a != 0; k_ladder.inc)
  static void scalar_mult_x(hipStream_t, const uint64_t* k, int k_stride, const uint64_t* x, const uint64_t* y, uint64_t* ox, uint64_t* scratch, size_t n, int flags);
  // k_affine_<curve>.hip
  static void to_affine_batched(hipStream_t, const uint64_t* jx, const uint64_t* jy, const uint64_t* jz, uint64_t* x, uint64_t* y, size_t n, bool in_fast_domain);
  static void inverse_batched(hipStream_t, const uint64_t* a, uint64_t* out, size_t n);
  static void x_mod_n_equals(hipStream_t, const uint64_t* x, const uint8_t* finite, const uint64_t* r, uint8_t* ok, size_t n);
  static void affine_add_batched(hipStream_t, const uint64_t* ax, const uint64_t* ay, const uint64_t* bx, const uint64_t* by, uint64_t* rx, uint64_t* ry, uint8_t* finite, size_t n);
  static void pack_table(hipStream_t, const uint64_t* tx, const uint64_t* ty, uint32_t* table);
  static void base_windowed(hipStream_t, const uint64_t* k, const uint32_t* table, uint64_t* ox, uint64_t* oy, uint64_t* oz, size_t n, bool constant_time);
  static void pack_table_signed(hipStream_t, int wbits, const uint64_t* tx, const uint64_t* ty, uint32_t* table);
  static void base_windowed_signed(hipStream_t, const uint64_t* k, const uint32_t* table, uint64_t* ox, uint64_t* oy, uint64_t* oz, size_t n, bool constant_time);
  static void pack_table_big(hipStream_t, const uint64_t* tx, const uint64_t* ty, uint32_t* table);
  static void base_windowed_big(hipStream_t, const uint64_t* k, const uint32_t* table, uint64_t* ox, uint64_t* oy, uint64_t* oz, size_t n);
  // k_varwin_<curve>.hip
  static void add_mixed_complete(hipStream_t, const uint64_t*, const uint64_t*, const uint64_t*, const uint64_t*, const uint64_t*, uint64_t*, uint64_t*, uint64_t*, size_t);
  static void varwin_scalar_mult(hipStream_t, const uint64_t* k, int k_stride, const uint64_t* x, const uint64_t* y, int flags, uint64_t* scratch, uint64_t* ox, uint64_t* oy, size_t n);
};
// k_msm_common.hip: the kernels of the bucket sums and the batch verifications that know no curve (msm_stages.cuh has the stages; PUBLIC data).  Every launcher
// enqueues ONE kernel.  zero: bytes, a multiple of 16.  flags_all: ok[0] = every one of the n bytes of flags (16-byte aligned) is 1; n = 0: 1.
void msm_zero(hipStream_t, void* words, size_t bytes);
void msm_scan(hipStream_t, const uint32_t* hist, uint32_t* start, uint32_t* cursor, size_t K);
void msm_scatter(hipStream_t, const uint64_t* kk, uint32_t* cursor, uint32_t* sorted, uint32_t* broken, size_t n, size_t T, int c, int windows);
void flags_all(hipStream_t, const uint8_t* flags, size_t n, uint8_t* ok);
// k_msm_<curve>.hip: R = sum k_i P_i by the bucket method and the point sum over lanes (k_msm.inc; PUBLIC data).  Jacobian arrays are three planes of `total`
// elements in the fast domain, Z = 0 at infinity.  Every launcher enqueues ONE kernel; capi.hip's msm_schedule_of decides the sizes from (n, bits, flags).
constexpr int MSM_TREE_FAN = 16;                 // elements a lane of the tree sum adds per launch
template <int C> struct msm_launch {
  static void digits(hipStream_t, const uint64_t* k, const uint64_t* x, const uint64_t* y, uint64_t* kk, uint64_t* px, uint64_t* py, uint32_t* hist, uint32_t* counter, size_t n,
                     int bits, int c, int windows);
  static void slices(hipStream_t, const uint32_t* sorted, const uint64_t* kk, const uint64_t* px, const uint64_t* py, const uint32_t* start, uint64_t* buckets, uint64_t* partial,
                     uint32_t* broken, size_t n, size_t T, size_t L, size_t slices, int c, size_t K);
  static void combine(hipStream_t, const uint32_t* start, uint64_t* buckets, const uint64_t* partial, uint32_t* broken, size_t L, size_t slices, int c, size_t K);
  static void chunks(hipStream_t, const uint64_t* buckets, uint64_t* out, size_t lanes, size_t per_window, int c, int m, size_t K);
  static void tree(hipStream_t, uint64_t* arr, size_t total, size_t count, size_t stride, size_t groups, size_t lanes, int fan);
  static void tree_affine(hipStream_t, const uint64_t* x, const uint64_t* y, bool validate, uint32_t* counter, uint64_t* out, size_t n, size_t lanes, int fan);
  static void sanitize(hipStream_t, const uint64_t* k, const uint64_t* x, const uint64_t* y, uint64_t* kk, uint64_t* sx, uint64_t* sy, uint32_t* counter, size_t n, int bits);
  static void finish(hipStream_t, const uint64_t* arr, size_t total, size_t stride, int windows, int c, const uint32_t* counter, uint64_t* rx, uint64_t* ry, uint8_t* finite,
                     uint32_t* invalid);
};
// k_schnorr_batch.hip: BIP-340 batch verification (include/ecsimd_schnorr_batch.h; PUBLIC data).  Every launcher enqueues ONE kernel.  The call's header block in
// the workspace: the seed, the two sums as msm_launch::finish writes them (0: sum a R, 1: the key sum with the G term), the malformed lanes' counter.  192 bytes.
constexpr int BATCH_FAN = 16;                    // batch_tree.cuh, both batch verifications: children per node of the hash tree, terms per lane of the tree of additions
struct schnorr_batch_head { uint64_t seed[4], rx[2][4], ry[2][4]; uint32_t malformed, invalid[2]; uint8_t finite[2], unused[18]; };
// front: E = the challenge digest, leaf, (Px, Py) and (Rx, Ry) = the even-y lifts ((0, 0) on a malformed lane, which is counted in head->malformed), valid.
// node: out[j] = H_node(in[16 j ..]) for j < ceil(count / 16).  seed: head->seed from the root and n.  scalars: a, a e mod n, a s mod n (0 where not valid).
// sum: out[j] = sum of in[16 j ..] mod n; with gx (count <= 16): out[0] = n - sum (0 stays 0) and (gx, gy)[0] = G.  accept: ok[0] from head.
void schnorr_batch_front(hipStream_t, const words8& order, const uint64_t* px, const uint64_t* r, const uint64_t* s, const uint8_t* msg, size_t msg_bytes, size_t stride_bytes,
                         uint64_t* E, uint64_t* leaf, uint64_t* Px, uint64_t* Py, uint64_t* Rx, uint64_t* Ry, uint8_t* valid, schnorr_batch_head* head, size_t n);
void schnorr_batch_node(hipStream_t, const uint64_t* in, size_t count, uint64_t* out);
void schnorr_batch_seed(hipStream_t, const uint64_t* root, size_t n, schnorr_batch_head* head);
void schnorr_batch_scalars(hipStream_t, const gmod& order, const schnorr_batch_head* head, const uint64_t* E, const uint64_t* s, const uint8_t* valid, uint64_t* a, uint64_t* ae,
                           uint64_t* as, size_t n);
void schnorr_batch_sum(hipStream_t, const gmod& order, const uint64_t* in, size_t count, uint64_t* out, uint64_t* gx, uint64_t* gy);
void schnorr_batch_accept(hipStream_t, const schnorr_batch_head* head, uint8_t* ok);
// k_msm_ed25519.hip: the bucket method on the twisted Edwards curve and Ed25519 batch verification (include/ecsimd_ed25519_batch.h; PUBLIC data).  Every launcher
// enqueues ONE kernel.  The sum's stages are msm_stages.cuh's on ed25519.cuh's arithmetic.  Terms: k = n x 32 little-endian bytes, pts = n x 32-byte encodings, both at any alignment; kk = the masked scalars, pre = the decoded terms as
// three planes of n (y + x, y - x, 2 d x y); buckets, partial and the tree are FOUR planes (X, Y, Z, T), the identity (0, 1, 1, 0).  finish: out = the 32-byte
// encoding, or with raw != nullptr the extended point as 16 words at raw and no encoding.
// The batch's header block in the workspace: the seed, the two sums as finish writes them raw (0: sum z R, 1: the key sum with the B term), the malformed lanes'
// counter.  304 bytes.
struct ed25519_batch_head { uint64_t seed[4], sum[2][16]; uint32_t malformed, invalid[2]; uint8_t finite[2], unused[2]; };
struct ed25519_msm_launch {                      // msm_launch's shape: capi.hip's bucket_sum_run takes either
  static void digits(hipStream_t, const uint8_t* k, const uint8_t* pts, uint64_t* kk, uint64_t* pre, uint32_t* hist, uint32_t* counter, size_t n, int bits, int c, int windows);
  static void slices(hipStream_t, const uint32_t* sorted, const uint64_t* kk, const uint64_t* pre, const uint32_t* start, uint64_t* buckets, uint64_t* partial, uint32_t* broken,
                     size_t n, size_t T, size_t L, size_t slices, int c, size_t K);
  static void combine(hipStream_t, const uint32_t* start, uint64_t* buckets, const uint64_t* partial, uint32_t* broken, size_t L, size_t slices, int c, size_t K);
  static void chunks(hipStream_t, const uint64_t* buckets, uint64_t* out, size_t lanes, size_t per_window, int c, int m, size_t K);
  static void tree(hipStream_t, uint64_t* arr, size_t total, size_t count, size_t stride, size_t groups, size_t lanes, int fan);
  static void finish(hipStream_t, const uint64_t* arr, size_t total, size_t stride, int windows, int c, const uint32_t* counter, uint8_t* out, uint64_t* raw, uint8_t* finite,
                     uint32_t* invalid);
};
// k_bls12_381.hip (G = g1_curve) and k_bls12_381_g2.hip (G = g2_curve): BLS12-381 G1 and G2 (include/ecsimd_bls12_381.h, include/ecsimd_bls12_381_g2.h; g1.cuh,
// g2.cuh, the kernels' one text k_bls12_381.inc; PUBLIC data).  Every launcher enqueues ONE kernel.  A field element is R = 1 (Fp) or 2 (Fp2) 48-byte components.  Points
// cross as the standard uncompressed (96 R bytes: pts) or compressed (48 R bytes) encodings at any alignment, scalars as n x 8 words, 16-byte aligned.  A field
// element in the workspace is 48 R bytes: its components least significant first, each twelve little-endian words in Montgomery form, element e of an array at
// byte 48 R e; a Jacobian array of `total` elements is X, Y, Z one behind the other (X at e, Y at total + e, Z at 2 total + e), Z = 0 the identity; px, py = the
// decoded terms' x and y (n elements each).  Raw records are 48 bytes; a field operand is R records, least significant first, a point x, y and one flag record.
enum bls381_raw_op { BLS381_RAW_FE_MUL = 0, BLS381_RAW_FE_SQR = 1, BLS381_RAW_FE_ADD = 2, BLS381_RAW_FE_SUB = 3, BLS381_RAW_FE_NEG = 4, BLS381_RAW_FE_INVERT = 5,
                     BLS381_RAW_FE_SQRT = 6, BLS381_RAW_FE_CANON = 7, BLS381_RAW_POINT_ADD = 8, BLS381_RAW_POINT_DBL = 9, BLS381_RAW_POINT_MADD = 10 };
constexpr int bls381_raw_inputs(int op, int R) {
  return op == BLS381_RAW_POINT_ADD ? 4 * R + 2 : op == BLS381_RAW_POINT_MADD ? 4 * R + 1 : op == BLS381_RAW_POINT_DBL ? 2 * R + 1
       : (op == BLS381_RAW_FE_MUL || op == BLS381_RAW_FE_ADD || op == BLS381_RAW_FE_SUB) ? 2 * R : R;
}
constexpr int bls381_raw_outputs(int op, int R) { return op >= BLS381_RAW_POINT_ADD ? 2 * R + 1 : op == BLS381_RAW_FE_SQRT ? R + 1 : R; }
template <class G> struct bls381_launch {        // from digits on msm_launch's shape: capi.hip's bucket_sum_run takes it
  static void decompress(hipStream_t, const uint8_t* in, uint8_t* out, uint8_t* ok, size_t n);
  static void compress(hipStream_t, const uint8_t* in, uint8_t* out, uint8_t* ok, size_t n);
  static void check(hipStream_t, const uint8_t* in, uint8_t* on_curve, uint8_t* in_subgroup, size_t n);
  static void mul(hipStream_t, const uint64_t* k, const uint8_t* in, uint8_t* out, uint8_t* ok, size_t n);
  static void raw(hipStream_t, int op, const uint8_t* in, uint8_t* out, size_t n);
  static void digits(hipStream_t, const uint64_t* k, const uint8_t* pts, uint64_t* kk, uint64_t* px, uint64_t* py, uint32_t* hist, uint32_t* counter, size_t n, int bits, int c,
                     int windows);
  static void slices(hipStream_t, const uint32_t* sorted, const uint64_t* kk, const uint64_t* px, const uint64_t* py, const uint32_t* start, uint64_t* buckets, uint64_t* partial,
                     uint32_t* broken, size_t n, size_t T, size_t L, size_t slices, int c, size_t K);
  static void combine(hipStream_t, const uint32_t* start, uint64_t* buckets, const uint64_t* partial, uint32_t* broken, size_t L, size_t slices, int c, size_t K);
  static void chunks(hipStream_t, const uint64_t* buckets, uint64_t* out, size_t lanes, size_t per_window, int c, int m, size_t K);
  static void tree(hipStream_t, uint64_t* arr, size_t total, size_t count, size_t stride, size_t groups, size_t lanes, int fan);
  // out[g] = the sum of the valid points g, g + lanes, ... (fan of them) of n encodings, the compressed ones where `compressed`; malformed ones are counted and skipped
  static void tree_affine(hipStream_t, const uint8_t* pts, bool compressed, uint32_t* counter, uint64_t* out, size_t n, size_t lanes, int fan);
  // the LANES route's front: out[i] = (k[i] mod 2^bits) P[i] as a Jacobian array of n; a malformed point is counted and gives the identity
  static void products(hipStream_t, const uint64_t* k, const uint8_t* pts, uint32_t* counter, uint64_t* out, size_t n, int bits);
  static void finish(hipStream_t, const uint64_t* arr, size_t total, size_t stride, int windows, int c, const uint32_t* counter, uint8_t* out, uint8_t* finite, uint32_t* invalid);
};
// front: h = SHA-512(R || A || M) mod L, leaf, A and R copied to Aenc / Renc, valid = s < L (&& no small-order A or R); a lane that is not valid counts in
// head->malformed.  node / seed: schnorr_batch's shapes under this call's tags.  scalars: z, and where zh is given z h mod L and z s mod L (0 where not valid).
// sum: out[j] = sum of in[16 j ..] mod L; with benc (count <= 16): out[0] = L - sum (0 stays 0) and benc[0] = B's encoding.  accept: ok[0] from head.
void ed25519_batch_front(hipStream_t, const gmod& L, const uint8_t* pk, const uint8_t* sig, const uint8_t* msg, size_t msg_bytes, size_t stride_bytes, const uint32_t* lens,
                         bool reject_small_order, uint64_t* h, uint64_t* leaf, uint64_t* Aenc, uint64_t* Renc, uint8_t* valid, ed25519_batch_head* head, size_t n);
void ed25519_batch_node(hipStream_t, const uint64_t* in, size_t count, uint64_t* out);
void ed25519_batch_seed(hipStream_t, const uint64_t* root, size_t n, ed25519_batch_head* head);
void ed25519_batch_scalars(hipStream_t, const gmod& L, const ed25519_batch_head* head, const uint64_t* h, const uint8_t* sig, const uint8_t* valid, uint64_t* z, uint64_t* zh,
                           uint64_t* zs, size_t n);
void ed25519_batch_sum(hipStream_t, const gmod& L, const uint64_t* in, size_t count, uint64_t* out, uint64_t* benc);
void ed25519_batch_accept(hipStream_t, const ed25519_batch_head* head, uint8_t* ok);
// The per-lane cofactored rule: front writes valid = s < L && A and R decode (&& no small-order A or R), s, h, R's affine (x, y) as two planes of n and the table
// of 1 .. 8 times -A (ed25519_table_bytes(n) bytes); loop ok = valid && [8]([s]B - [h]A - R) is the identity.
void ed25519_cofactored_front(hipStream_t, const gmod& L, const uint8_t* pk, const uint8_t* sig, const uint8_t* msg, size_t msg_bytes, size_t stride_bytes, const uint32_t* lens,
                              bool reject_small_order, uint64_t* s, uint64_t* h, uint64_t* rxy, void* table, uint8_t* valid, size_t n);
void ed25519_cofactored_loop(hipStream_t, const uint64_t* s, const uint64_t* h, const uint64_t* rxy, const void* table, const uint8_t* valid, uint8_t* ok, size_t n);

// k_sm2.hip: SM3 and the SM2 signature scheme around the generic curve kernels.  sm2_curve_words: the curve's classical a, b, x_G, y_G as Z_A hashes them.
// lens may be null (every lane has msg_bytes bytes); id_stride = 0: one ID for the whole batch; id_bytes <= 8191; msg_bytes < 2^31.
struct sm2_curve_words { words8 a, b, gx, gy; };
void sm3(hipStream_t, const uint8_t* msg, size_t msg_bytes, size_t stride_bytes, const uint32_t* lens, uint64_t* e, size_t n);
void sm2_za(hipStream_t, const sm2_curve_words&, const uint64_t* qx, const uint64_t* qy, const uint8_t* id, size_t id_bytes, size_t id_stride, uint64_t* za, size_t n);
void sm2_digest(hipStream_t, const sm2_curve_words&, const uint64_t* qx, const uint64_t* qy, const uint8_t* id, size_t id_bytes, size_t id_stride, const uint8_t* msg, size_t msg_bytes,
                size_t stride_bytes, const uint32_t* lens, uint64_t* e, size_t n);
void sm2_verify_scalars(hipStream_t, const words8& order, const uint64_t* r, const uint64_t* s, uint64_t* u1, uint64_t* u2, uint8_t* valid, size_t n);
void sm2_accept(hipStream_t, const words8& order, const uint64_t* e, const uint64_t* x, const uint8_t* finite, const uint64_t* r, const uint8_t* valid, uint8_t* ok, size_t n);
void sm2_sign_scalars(hipStream_t, const gmod& N, const uint64_t* e, const uint64_t* d, const uint64_t* k, const uint64_t* x, uint64_t* r, uint64_t* s, uint8_t* ok, size_t n);   // SECRET d, k
void sm2_key_range(hipStream_t, const gmod& N, const uint64_t* d, uint64_t* qx, uint64_t* qy, uint8_t* ok, size_t n);                                                             // SECRET d
inline size_t scalar_mult_x_scratch_bytes(size_t n) { return 4 * n * 32 + ((n + 31) & ~(size_t)31); }   // odd scalars, num, den, 1/den, zero flags
// The 4-bit fixed-base table in LDS (BASELINE configs[2]): odd digits only (round 3) -- the regular recoding of the odd one of k mod n, n - k, as in
// the big-window kernel: 64 windows x 8 odd multiples (2d + 1) 16^w G = 32 KiB, 63 mixed additions, no zero digit and therefore no "skip" / "infinity"
// selects.  The signed 5- / 7-bit LDS tables use the same odd digits: 52 / 37 windows x 16 / 64 odd multiples (2d + 1) 2^(bits w) G, no carry window.
// (Round 1's unsigned 4-bit digits and carry-recoded signed digits were measured against these and removed.)
constexpr int FIXED4_ENTRIES = 8;
constexpr size_t WINDOW_TABLE_BYTES = 64 * FIXED4_ENTRIES * 64;   // 64 windows x entries x (x, y)

// k_ntt.hip: the number-theoretic transform over a registered prime field (include/ecsimd_ntt.h; ntt.cuh has the schedule and the pass body).  Every launcher
// enqueues ONE kernel.  ntt_pass: ntt::tiles_of(A.G) workgroups of ntt::LANES; ntt_bitrev: out[rev(i)] = in[i] per array of 2^log_n elements, out may be in.
void ntt_pass(hipStream_t, const gmod& M, const ntt::pass_args& A);
void ntt_bitrev(hipStream_t, const uint64_t* in, uint64_t* out, int log_n, size_t batch);

}  // namespace launch
}  // namespace ecsimd_hip
