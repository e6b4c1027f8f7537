/* p384_caller.c -- a C99 caller of include/ecsimd_p384.h: every prototype used once, so the header compiles as plain C and the symbols resolve at link
 * time.  tests/test_p384_cpu.py builds it with -std=c99 -pedantic -Werror; nothing here runs on a device. */
#include "ecsimd_p384.h"
#include <stddef.h>

int main(int argc, char** argv) {
  uint8_t* b = NULL;
  (void)argv;
  if (argc > 1000) { /* never taken */
    int rc = ecsimd_p384_sha384(NULL, b, 0, 0, NULL, b, 0);
    rc |= ecsimd_p384_pubkey(NULL, b, b, b, 0);
    rc |= ecsimd_p384_ecdh(NULL, b, b, b, b, 0);
    rc |= ecsimd_p384_ecdsa_verify(NULL, b, b, b, b, 0);
    rc |= ecsimd_p384_ecdsa_sign(NULL, b, b, b, b, 0, 0);
    rc |= ecsimd_p384_raw(NULL, ECSIMD_P384_RAW_DOUBLE_MULT, b, b, 0);
    return rc + ecsimd_p384_raw_inputs(ECSIMD_P384_RAW_FE_MUL) + ecsimd_p384_raw_outputs(ECSIMD_P384_RAW_BASE_MULT);
  }
  return 0;
}
