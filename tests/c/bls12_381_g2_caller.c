/* bls12_381_g2_caller.c -- a C99 caller of include/ecsimd_bls12_381_g2.h: every prototype used once, so the header compiles as plain C and the symbols resolve
 * at link time.  tests/test_cpp_bls12_381_g2.py builds it with -std=c99 -pedantic -Werror; nothing here runs on a device. */
#include "ecsimd_bls12_381_g2.h"
#include <stddef.h>

int main(int argc, char** argv) {
  uint8_t* b = NULL;
  uint64_t* k = NULL;
  uint32_t* c = NULL;
  ecsimd_msm_plan_t plan;
  (void)argv;
  if (argc > 1000) { /* never taken */
    int rc = ecsimd_bls381_g2_decompress(NULL, b, b, b, 0);
    rc |= ecsimd_bls381_g2_compress(NULL, b, b, b, 0);
    rc |= ecsimd_bls381_g2_check(NULL, b, b, b, 0);
    rc |= ecsimd_bls381_g2_mul(NULL, k, b, b, b, 0);
    rc |= ecsimd_bls381_g2_msm(NULL, k, b, b, b, c, 0, 255, ECSIMD_MSM_ALG_AUTO);
    rc |= ecsimd_bls381_g2_point_sum(NULL, b, b, b, c, 0, ECSIMD_BLS381_G2_COMPRESSED);
    rc |= ecsimd_bls381_g2_msm_plan(ECSIMD_BLS381_G2_MSM_AUTO_THRESHOLD, 255, ECSIMD_MSM_ALG_BUCKETS, &plan);
    rc |= ecsimd_bls381_g2_raw(NULL, ECSIMD_BLS381_G2_RAW_POINT_MADD, b, b, 0);
    return rc + ecsimd_bls381_g2_raw_inputs(ECSIMD_BLS381_G2_RAW_FE2_MUL) + ecsimd_bls381_g2_raw_outputs(ECSIMD_BLS381_G2_RAW_FE2_SQRT);
  }
  return 0;
}
