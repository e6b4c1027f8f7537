// k_bls12_381_g2.hip -- BLS12-381 G2: k_bls12_381.inc's kernels over g2.cuh (E'(Fp2) on fp2.cuh), behind ecsimd_bls381_g2_* (include/ecsimd_bls12_381_g2.h).
//
// INLINING: g2_dbl, g2_add and g2_madd are OUT OF LINE, compiled ONCE in this unit, and every kernel calls them, as do their own nested uses.  The G1 unit inlines
// everything, and its k_g1_chunks alone is 117 445 VALU instructions; at three Fp products per Fp2 product the same policy would make this unit several times the
// size of every other unit together, for nothing: a call moves two 72-word points through private memory around roughly 48 Fp products of work.  Everything
// below the three operations (fp2.cuh, fe381.cuh) stays inlined into them.  DESIGN.md 4n has the listing's numbers.
#define G2_DBL BLS381_OUT_OF_LINE
#define G2_ADD BLS381_OUT_OF_LINE
#define G2_MADD BLS381_OUT_OF_LINE                  // bls381_curve.inc, INLINING POLICY
#include "g2.cuh"
#include "bls381_bytes.cuh"

// THE RAW KERNEL is this unit's own, not k_bls12_381.inc's: a diagnostic, written in two forms (G1's converts its six records up front, G2's as it needs them),
// and either form moves the other unit's listing.
namespace ecsimd_hip {
namespace {
using launch::BLOCK;
#define GID size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x; if (i >= n) return
// one function of the layers on raw 48-byte records (launch::bls381_raw_inputs / _outputs of them per lane at R = 2; an Fp2 operand is two records, c0 then c1); every
// 384-bit value is the residue it represents
ECS_DEV void raw2_store(uint8_t* __restrict__ p, const fp2& v, uint32_t aligned) { be48_store(p, fe381_from_mont(v.c0), aligned); be48_store(p + 48, fe381_from_mont(v.c1), aligned); }
__global__ void __launch_bounds__(BLOCK) k_bls381_g2_raw(int op, const uint8_t* __restrict__ in, uint8_t* __restrict__ out, uint32_t aligned, size_t n) {
  GID;
  const int ni = launch::bls381_raw_inputs(op, 2), no = launch::bls381_raw_outputs(op, 2);
  const uint8_t* ip = in + (size_t)48 * ni * i;
  uint8_t* op_ = out + (size_t)48 * no * i;
  const auto rec = [&](int j) { return j < ni ? fe381_to_mont(be48_load(ip + 48 * j, aligned)) : fe381_zero(); };
  const fp2 a = {rec(0), rec(1)}, b = {rec(2), rec(3)};
  if (op < launch::BLS381_RAW_POINT_ADD) {
    fp2 r = a;
    switch (op) {
      case launch::BLS381_RAW_FE_MUL: r = fp2_mul(a, b); break;
      case launch::BLS381_RAW_FE_SQR: r = fp2_sqr(a); break;
      case launch::BLS381_RAW_FE_ADD: r = fp2_add(a, b); break;
      case launch::BLS381_RAW_FE_SUB: r = fp2_sub(a, b); break;
      case launch::BLS381_RAW_FE_NEG: r = fp2_neg(a); break;
      case launch::BLS381_RAW_FE_INVERT: r = fp2_invert(a); break;
      case launch::BLS381_RAW_FE_SQRT: {
        bool ok;
        r = fp2_sqrt(a, ok);
        be48_store(op_ + 96, fe384_small(ok ? 1u : 0u), aligned);
        break; }
      default: break;                                                   // FE_CANON
    }
    raw2_store(op_, r, aligned);
    return;
  }
  // x1 = a, y1 = b, id1 = record 4; the second operand from record 5 on
  const g2_point p1 = (fe381_from_mont(rec(4)).w[0] & 1u) ? g2_identity() : g2_from_affine({a, b});
  const g2_affine q2 = {{rec(5), rec(6)}, {rec(7), rec(8)}};
  g2_point R;
  if (op == launch::BLS381_RAW_POINT_ADD) R = g2_add(p1, (fe381_from_mont(rec(9)).w[0] & 1u) ? g2_identity() : g2_from_affine(q2));
  else if (op == launch::BLS381_RAW_POINT_DBL) R = g2_dbl(p1);
  else R = g2_madd(p1, q2);
  const bool id = g2_is_identity(R);
  g2_affine q = {fp2_zero(), fp2_zero()};
  if (!id) q = g2_to_affine(R);
  raw2_store(op_, q.x, aligned); raw2_store(op_ + 96, q.y, aligned);
  be48_store(op_ + 192, fe384_small(id ? 1u : 0u), aligned);
}

#undef GID
}  // namespace
}  // namespace ecsimd_hip
#define BLS381_K(stage) k_g2_##stage
#define BLS381_K_RAW k_bls381_g2_raw
#define BLS381_LAUNCH bls381_launch<g2_curve>
#include "k_bls12_381.inc"
