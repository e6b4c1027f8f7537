// p384_host_check.cpp -- fe384.cuh / p384.cuh on the HOST: the reduction, the scalar field, the complete group law and the three window loops as the
// kernels run them, with the column multiply-add in plain C++ (fe384_mac's host branch).  tests/test_p384_cpu.py feeds it operands and compares the answers
// with Python integers and tools/p384_model.py.  No GPU is involved: this checks the logic every 384-bit kernel shares before a device ever runs it.
//
// stdin: one request per line, "<op> <96 hex digits> ..."; stdout: the results as 96 hex digits each, space-separated.
//   mul a b | sqr a | add a b | sub a b | neg a | inv a | canon a | scmul a b | scinv a
//   valid x y                     -> flag
//   padd x1 y1 id1 x2 y2 id2      -> x y id   (Algorithm 4 on the two points; id = 1: the identity, coordinates ignored)
//   pdbl x y id                   -> x y id
//   base k | var k x y | dmul u1 u2 x y  -> x y id   (scalars are reduced modulo n first)
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>
#include <string>
#include <vector>

#include "../../ecsimd_amd/csrc/p384.cuh"

using namespace ecsimd_hip;

static const uint32_t HOST_BASE[P384_BASE_WINDOWS * P384_BASE_ENTRIES * 24] = {P384_BASE_TABLE};

static fe384 parse(const char* s) {
  fe384 r;
  for (int j = 0; j < 12; ++j) { unsigned v = 0; sscanf(s + 8 * j, "%8x", &v); r.w[11 - j] = v; }
  return r;
}
static void show(const fe384& a) {
  for (int j = 11; j >= 0; --j) printf("%08x", a.w[j]);
  printf(" ");
}
static void show_point(const p384_point& p) {
  const p384_affine a = p384_to_affine(p);
  show(a.x); show(a.y); show(fe384_small(p384_is_identity(p) & 1u));
}
static p384_point point_of(const fe384& x, const fe384& y, const fe384& id) {
  return id.w[0] ? p384_identity() : p384_from_affine({fe384_canon(x), fe384_canon(y)});
}

int main() {
  char line[2048];
  std::vector<uint32_t> table(P384_TABLE_WORDS);
  while (fgets(line, sizeof line, stdin)) {
    std::vector<fe384> a;
    char* tok = strtok(line, " \n");
    if (!tok) continue;
    const std::string op = tok;
    while ((tok = strtok(nullptr, " \n"))) a.push_back(parse(tok));
    if (op == "mul") show(fe384_mul(fe384_canon(a[0]), fe384_canon(a[1])));
    else if (op == "sqr") show(fe384_sqr(fe384_canon(a[0])));
    else if (op == "add") show(fe384_add(fe384_canon(a[0]), fe384_canon(a[1])));
    else if (op == "sub") show(fe384_sub(fe384_canon(a[0]), fe384_canon(a[1])));
    else if (op == "neg") show(fe384_neg(fe384_canon(a[0])));
    else if (op == "inv") show(fe384_invert(fe384_canon(a[0])));
    else if (op == "canon") show(fe384_canon(a[0]));
    else if (op == "scmul") show(sc384_mul(sc384_reduce(a[0]), sc384_reduce(a[1])));
    else if (op == "scinv") show(sc384_invert(sc384_reduce(a[0])));
    else if (op == "valid") show(fe384_small(p384_valid({a[0], a[1]}) & 1u));
    else if (op == "padd") show_point(p384_add(point_of(a[0], a[1], a[2]), point_of(a[3], a[4], a[5])));
    else if (op == "pdbl") show_point(p384_dbl(point_of(a[0], a[1], a[2])));
    else if (op == "base") show_point(p384_base_ct(sc384_reduce(a[0]), HOST_BASE));
    else if (op == "var") {
      p384_table_build(table.data(), 1, 0, p384_from_affine({a[1], a[2]}));
      show_point(p384_var_ct(sc384_reduce(a[0]), table.data(), 1, 0));
    } else if (op == "dmul") {
      p384_table_build(table.data(), 1, 0, p384_from_affine({a[2], a[3]}));
      const p384_point R = p384_double_mult(sc384_reduce(a[0]), sc384_reduce(a[1]), HOST_BASE, table.data(), 1, 0);
      show_point(R);
    } else { fprintf(stderr, "unknown op %s\n", op.c_str()); return 2; }
    printf("\n");
  }
  return 0;
}
