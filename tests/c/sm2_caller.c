/* sm2_caller.c -- a C99 caller of include/ecsimd_sm2.h: every prototype used once, so the header compiles as plain C and the symbols resolve at link
 * time.  tests/test_sm2_cpu.py builds it with -std=c99 -pedantic -Werror; nothing here runs on a device. */
#include "ecsimd_sm2.h"
#include <stddef.h>

int main(int argc, char** argv) {
  uint8_t* b = NULL;
  uint64_t* w = NULL;
  uint32_t* lens = NULL;
  (void)argv;
  if (argc > 1000) { /* never taken */
    int curve = 0;
    int rc = ecsimd_sm2_curve(&curve);
    rc |= ecsimd_sm2_sm3(NULL, b, 0, 0, lens, w, 0);
    rc |= ecsimd_sm2_za(NULL, curve, w, w, b, 16, 0, w, 0);
    rc |= ecsimd_sm2_digest(NULL, curve, w, w, b, 16, 0, b, 0, 0, lens, w, 0);
    rc |= ecsimd_sm2_pubkey(NULL, curve, w, w, w, b, 0);
    rc |= ecsimd_sm2_verify_digest(NULL, curve, w, w, w, w, w, b, 0);
    rc |= ecsimd_sm2_verify(NULL, curve, w, w, b, 16, 0, b, 0, 0, lens, w, w, b, 0);
    rc |= ecsimd_sm2_sign_digest(NULL, curve, w, w, NULL, w, w, b, 0, 0);
    return rc;
  }
  return 0;
}
