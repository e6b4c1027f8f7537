// k_bls12_381.hip -- BLS12-381 G1: k_bls12_381.inc's kernels over g1.cuh (E(Fp) on fe381.cuh), behind ecsimd_bls12_381_g1_* and ecsimd_bls12_381_raw
// (include/ecsimd_bls12_381.h).
//
// INLINING: everything, the three point operations included (g1.cuh's default).  k_g1_chunks alone is 117 445 VALU instructions that way, and no kernel that
// holds ONE mixed addition needs scratch for it except k_g1_slices (DESIGN.md 4m has the listing's numbers).
#include "g1.cuh"
#include "bls381_bytes.cuh"

// THE RAW KERNEL is this unit's own, not k_bls12_381.inc's: a diagnostic, written in two forms (G1's converts its six records up front, G2's as it needs them),
// and either form moves the other unit's listing.
namespace ecsimd_hip {
namespace {
using launch::BLOCK;
#define GID size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x; if (i >= n) return
// one function of the layers on raw 48-byte records (launch::bls381_raw_inputs / _outputs of them per lane at R = 1); every 384-bit value is the residue it represents
__global__ void __launch_bounds__(BLOCK) k_bls381_raw(int op, const uint8_t* __restrict__ in, uint8_t* __restrict__ out, uint32_t aligned, size_t n) {
  GID;
  const int ni = launch::bls381_raw_inputs(op, 1), no = launch::bls381_raw_outputs(op, 1);
  const uint8_t* ip = in + (size_t)48 * ni * i;
  uint8_t* op_ = out + (size_t)48 * no * i;
  fe381 a[6];
#pragma unroll
  for (int j = 0; j < 6; ++j) a[j] = j < ni ? fe381_to_mont(be48_load(ip + 48 * j, aligned)) : fe381_zero();
  if (op < launch::BLS381_RAW_POINT_ADD) {
    fe381 r = a[0];
    switch (op) {
      case launch::BLS381_RAW_FE_MUL: r = fe381_mul(a[0], a[1]); break;
      case launch::BLS381_RAW_FE_SQR: r = fe381_sqr(a[0]); break;
      case launch::BLS381_RAW_FE_ADD: r = fe381_add(a[0], a[1]); break;
      case launch::BLS381_RAW_FE_SUB: r = fe381_sub(a[0], a[1]); break;
      case launch::BLS381_RAW_FE_NEG: r = fe381_neg(a[0]); break;
      case launch::BLS381_RAW_FE_INVERT: r = fe381_invert(a[0]); break;
      case launch::BLS381_RAW_FE_SQRT: {
        bool ok;
        r = fe381_sqrt(a[0], ok);
        be48_store(op_ + 48, fe384_small(ok ? 1u : 0u), aligned);
        break; }
      default: break;                                                   // FE_CANON
    }
    be48_store(op_, fe381_from_mont(r), aligned);
    return;
  }
  const g1_point p1 = (fe381_from_mont(a[2]).w[0] & 1u) ? g1_identity() : g1_from_affine({a[0], a[1]});
  g1_point R;
  if (op == launch::BLS381_RAW_POINT_ADD) R = g1_add(p1, (fe381_from_mont(a[5]).w[0] & 1u) ? g1_identity() : g1_from_affine({a[3], a[4]}));
  else if (op == launch::BLS381_RAW_POINT_DBL) R = g1_dbl(p1);
  else R = g1_madd(p1, a[3], a[4]);
  const bool id = g1_is_identity(R);
  g1_affine q = {fe381_zero(), fe381_zero()};
  if (!id) q = g1_to_affine(R);
  be48_store(op_, fe381_from_mont(q.x), aligned);
  be48_store(op_ + 48, fe381_from_mont(q.y), aligned);
  be48_store(op_ + 96, fe384_small(id ? 1u : 0u), aligned);
}

#undef GID
}  // namespace
}  // namespace ecsimd_hip
#define BLS381_K(stage) k_g1_##stage
#define BLS381_K_RAW k_bls381_raw
#define BLS381_LAUNCH bls381_launch<g1_curve>
#include "k_bls12_381.inc"
