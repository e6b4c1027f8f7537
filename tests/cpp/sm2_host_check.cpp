// sm2_host_check.cpp -- sm3.cuh on the HOST: the compression, the message walkers, the Z_A stream and the integer rules of SM2 verification as the kernels
// run them.  tests/test_sm2_cpu.py feeds it the boundary lengths and the edge scalars and compares the answers with tools/sm2_model.py and Python integers.
// No GPU is involved.
//
// stdin: one request per line; "-" stands for an empty byte string; stdout: the results as hex, space-separated.
//   sm3 <aligned> <offset> <msg>          -> digest      (the message lies `offset` bytes into a buffer that ENDS with it: nothing behind it exists)
//   after32 <aligned> <offset> <z> <msg>  -> digest      (SM3(z || msg), z = 32 bytes)
//   za <id> <t>                           -> digest      (SM3(ENTL || id || t), t = 192 bytes)
//   vs <r> <s> <n>                        -> valid u1 u2
//   acc <e> <x> <r> <n>                   -> flag
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>

#include "../../ecsimd_amd/csrc/sm3.cuh"

using namespace ecsimd_hip;

static std::vector<uint8_t> bytes_of(const std::string& h) {
  std::vector<uint8_t> r;
  if (h == "-") return r;
  for (size_t i = 0; i + 1 < h.size(); i += 2) r.push_back((uint8_t)strtoul(h.substr(i, 2).c_str(), nullptr, 16));
  return r;
}
static sm2_int int_of(const std::string& h) {
  sm2_int r;
  for (int j = 0; j < 8; ++j) r.w[7 - j] = (uint32_t)strtoul(h.substr(8 * j, 8).c_str(), nullptr, 16);
  return r;
}
static void show(const uint32_t (&be)[8]) {
  for (int j = 0; j < 8; ++j) printf("%08x", be[j]);
  printf(" ");
}
static void show(const sm2_int& a) {
  for (int j = 7; j >= 0; --j) printf("%08x", a.w[j]);
  printf(" ");
}
// a 4-byte aligned block that ends with `msg`, the message `offset` bytes behind an aligned address
struct placed { std::vector<uint32_t> store; const uint8_t* at; };
static placed place(const std::vector<uint8_t>& msg, size_t offset) {
  placed p;
  const size_t total = offset + msg.size();
  p.store.assign((total + 3) / 4 + 1, 0xa5a5a5a5u);
  uint8_t* base = reinterpret_cast<uint8_t*>(p.store.data());
  if (!msg.empty()) memcpy(base + offset, msg.data(), msg.size());
  p.at = base + offset;
  return p;
}

int main() {
  static char line[70000];
  alignas(16) static uint32_t spare[8];
  while (fgets(line, sizeof line, stdin)) {
    std::vector<std::string> a;
    for (char* tok = strtok(line, " \n"); tok; tok = strtok(nullptr, " \n")) a.push_back(tok);
    if (a.empty()) continue;
    const std::string op = a[0];
    if (op == "sm3") {
      const placed p = place(bytes_of(a[3]), (size_t)atoi(a[2].c_str()));
      const uint32_t len = (uint32_t)bytes_of(a[3]).size();
      sm3_state s = sm3_iv();
      if (atoi(a[1].c_str())) sm3_absorb_message<true>(s, p.at, len, reinterpret_cast<const uint8_t*>(spare));
      else sm3_absorb_message<false>(s, p.at, len, reinterpret_cast<const uint8_t*>(spare));
      show(s.h);
    } else if (op == "after32") {
      const std::vector<uint8_t> z = bytes_of(a[3]);
      uint32_t zw[8];
      for (int j = 0; j < 8; ++j) zw[j] = ((uint32_t)z[4 * j] << 24) | ((uint32_t)z[4 * j + 1] << 16) | ((uint32_t)z[4 * j + 2] << 8) | z[4 * j + 3];
      const placed p = place(bytes_of(a[4]), (size_t)atoi(a[2].c_str()));
      const uint32_t len = (uint32_t)bytes_of(a[4]).size();
      sm3_state s = sm3_iv();
      if (atoi(a[1].c_str())) sm3_absorb_after32<true>(s, zw, p.at, len, reinterpret_cast<const uint8_t*>(spare));
      else sm3_absorb_after32<false>(s, zw, p.at, len, reinterpret_cast<const uint8_t*>(spare));
      show(s.h);
    } else if (op == "za") {
      const std::vector<uint8_t> id = bytes_of(a[1]), t = bytes_of(a[2]);
      uint32_t tw[48];
      for (int j = 0; j < 48; ++j) tw[j] = ((uint32_t)t[4 * j] << 24) | ((uint32_t)t[4 * j + 1] << 16) | ((uint32_t)t[4 * j + 2] << 8) | t[4 * j + 3];
      const placed p = place(id, 1);
      const sm3_state s = sm3_za(p.at, (uint32_t)id.size(), reinterpret_cast<const uint8_t*>(spare), tw);
      show(s.h);
    } else if (op == "vs") {
      sm2_int u1, u2;
      const uint32_t valid = sm2_verify_scalars(int_of(a[1]), int_of(a[2]), int_of(a[3]), u1, u2);
      printf("%u ", valid); show(u1); show(u2);
    } else if (op == "acc") {
      printf("%u ", sm2_accept(int_of(a[1]), int_of(a[2]), int_of(a[3]), int_of(a[4])));
    } else { fprintf(stderr, "unknown op %s\n", op.c_str()); return 2; }
    printf("\n");
  }
  return 0;
}
