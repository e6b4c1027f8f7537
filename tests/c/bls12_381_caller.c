/* bls12_381_caller.c -- a C99 caller of include/ecsimd_bls12_381.h: every prototype used once, so the header compiles as plain C and the symbols resolve at
 * link time.  tests/test_cpp_bls12_381.py builds it with -std=c99 -pedantic -Werror; nothing here runs on a device. */
#include "ecsimd_bls12_381.h"
#include <stddef.h>

int main(int argc, char** argv) {
  uint8_t* b = NULL;
  uint64_t* k = NULL;
  uint32_t* c = NULL;
  ecsimd_msm_plan_t plan;
  (void)argv;
  if (argc > 1000) { /* never taken */
    int rc = ecsimd_bls12_381_g1_decompress(NULL, b, b, b, 0);
    rc |= ecsimd_bls12_381_g1_compress(NULL, b, b, b, 0);
    rc |= ecsimd_bls12_381_g1_check(NULL, b, b, b, 0);
    rc |= ecsimd_bls12_381_g1_mul(NULL, k, b, b, b, 0);
    rc |= ecsimd_bls12_381_g1_msm(NULL, k, b, b, b, c, 0, 255, ECSIMD_MSM_ALG_AUTO);
    rc |= ecsimd_bls12_381_g1_point_sum(NULL, b, b, b, c, 0, ECSIMD_BLS12_381_COMPRESSED);
    rc |= ecsimd_bls12_381_g1_msm_plan(ECSIMD_BLS12_381_MSM_AUTO_THRESHOLD, 255, ECSIMD_MSM_ALG_BUCKETS, &plan);
    rc |= ecsimd_bls12_381_raw(NULL, ECSIMD_BLS12_381_RAW_POINT_MADD, b, b, 0);
    return rc + ecsimd_bls12_381_raw_inputs(ECSIMD_BLS12_381_RAW_FE_MUL) + ecsimd_bls12_381_raw_outputs(ECSIMD_BLS12_381_RAW_FE_SQRT);
  }
  return 0;
}
