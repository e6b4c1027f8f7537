/* bip39_caller.c -- ecsimd_hip_pbkdf2_hmac_sha512 and ecsimd_hip_bip39_seed from plain C99: the published BIP-39 vector (twelve words, passphrase TREZOR) on 70
 * lanes, its seed through both entry points -- bip39_seed, and pbkdf2_hmac_sha512 with the salt "mnemonicTREZOR" spelled out -- and the BIP-32 master key of it.
 * Build: gcc -std=c99 -pedantic -Wall -Werror -I include tests/c/bip39_caller.c -L ecsimd_amd -lecsimd_hip   (tests/test_bip39_cpu.py) */
#include <ecsimd_hip.h>

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define N 70
#define CHECK(call) do { int rc_ = (call); if (rc_ != ECSIMD_HIP_OK) { fprintf(stderr, "%s -> %d (%s)\n", #call, rc_, ctx ? ecsimd_hip_last_error(ctx) : ""); return 1; } } while (0)

int main(void) {
  ecsimd_hip_ctx* ctx = NULL;
  const char* sentence = "abandon abandon abandon abandon abandon abandon abandon abandon abandon abandon abandon about";
  const char* seed_hex = "c55257c360c07c72029aebc1b53c05ed0362ada38ead3e3e9efa3708e53495531f09a6987599d18264c1e1c92f2cf141630c7a3c4ab7c81b2f001698e7463b04";
  const uint64_t master_k[4] = {0x00330866f22ff184ull, 0x912fd1e756631b5aull, 0x5c79bc13875112efull, 0xcbedc75b0d6412c8ull};   /* little-endian limbs */
  const size_t len = strlen(sentence), stride = (len + 3) / 4 * 4;
  static uint8_t host[N * 128], seeds[N][64], again[N][64], ok_host[N];
  static uint64_t k_host[N][4];
  uint8_t *words = NULL, *salt = NULL, *seed = NULL, *seed2 = NULL, *ok = NULL;
  uint64_t *k = NULL, *c = NULL;
  char hex[129];
  size_t i; int j;

  if (stride > 128 || ECSIMD_HIP_PBKDF2_SLICE < 2048) { fprintf(stderr, "the sentence or the slice constant changed\n"); return 1; }
  for (i = 0; i < N; ++i) memcpy(host + i * stride, sentence, len);
  CHECK(ecsimd_hip_init(0, &ctx));
  CHECK(ecsimd_hip_malloc(ctx, (void**)&words, N * stride)); CHECK(ecsimd_hip_malloc(ctx, (void**)&salt, 16));
  CHECK(ecsimd_hip_malloc(ctx, (void**)&seed, N * 64)); CHECK(ecsimd_hip_malloc(ctx, (void**)&seed2, N * 64)); CHECK(ecsimd_hip_malloc(ctx, (void**)&ok, N));
  CHECK(ecsimd_hip_malloc(ctx, (void**)&k, N * 32)); CHECK(ecsimd_hip_malloc(ctx, (void**)&c, N * 32));
  CHECK(ecsimd_hip_memcpy_h2d(ctx, words, host, N * stride));
  CHECK(ecsimd_hip_memcpy_h2d(ctx, salt, "mnemonicTREZOR", 14));
  CHECK(ecsimd_hip_bip39_seed(ctx, words, len, stride, NULL, salt + 8, 6, 0, NULL, seed, N));                     /* one passphrase for the call */
  CHECK(ecsimd_hip_pbkdf2_hmac_sha512(ctx, words, len, stride, NULL, salt, 14, 0, NULL, 2048u, seed2, 64, 64, N));
  CHECK(ecsimd_hip_bip32_master(ctx, seed, 64, 64, k, c, ok, N));
  CHECK(ecsimd_hip_memcpy_d2h(ctx, seeds, seed, N * 64)); CHECK(ecsimd_hip_memcpy_d2h(ctx, again, seed2, N * 64));
  CHECK(ecsimd_hip_memcpy_d2h(ctx, k_host, k, N * 32)); CHECK(ecsimd_hip_memcpy_d2h(ctx, ok_host, ok, N));
  for (i = 0; i < N; ++i) {
    for (j = 0; j < 64; ++j) sprintf(hex + 2 * j, "%02x", seeds[i][j]);
    if (strcmp(hex, seed_hex) != 0) { fprintf(stderr, "lane %zu: seed %s\n", i, hex); return 1; }
    if (memcmp(seeds[i], again[i], 64) != 0) { fprintf(stderr, "lane %zu: pbkdf2_hmac_sha512 differs from bip39_seed\n", i); return 1; }
    if (!ok_host[i] || memcmp(k_host[i], master_k, 32) != 0) { fprintf(stderr, "lane %zu: master key\n", i); return 1; }
  }
  if (ecsimd_hip_bip39_seed(ctx, words, len, stride, NULL, NULL, 6, 0, NULL, seed, N) != ECSIMD_HIP_ERR_BAD_ARG) { fprintf(stderr, "a null passphrase of 6 bytes was accepted\n"); return 1; }
  CHECK(ecsimd_hip_free(ctx, words)); CHECK(ecsimd_hip_free(ctx, salt)); CHECK(ecsimd_hip_free(ctx, seed)); CHECK(ecsimd_hip_free(ctx, seed2)); CHECK(ecsimd_hip_free(ctx, ok));
  CHECK(ecsimd_hip_free(ctx, k)); CHECK(ecsimd_hip_free(ctx, c));
  CHECK(ecsimd_hip_destroy(ctx));
  printf("bip39_caller ok: %d seeds\n", N);
  return 0;
}
