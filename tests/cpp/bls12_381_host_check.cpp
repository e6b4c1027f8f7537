// bls12_381_host_check.cpp -- fe381.cuh / g1.cuh on the HOST: the Montgomery reduction, the group law with its branches, the scalar product, the subgroup test
// and the serialisation's rules as the kernels run them, with the column multiply-add in plain C++.  tests/test_bls12_381_cpu.py feeds it operands and
// compares the answers with Python integers and tools/bls12_381_model.py.  No GPU is involved: the logic is right before a device runs it.
//
// stdin: one request per line, "<op> <96 hex digits> ..."; stdout: the results as 96 hex digits each, space-separated.  Field operands are ANY 384-bit value.
//   mul a b | sqr a | add a b | sub a b | neg a | inv a | canon a   -> the plain residue
//   sqrt a                        -> root flag
//   lex a                         -> flag (a > (p - 1) / 2)
//   padd x1 y1 id1 x2 y2 id2      -> x y id    (id = 1: the identity, coordinates ignored; points are NOT validated)
//   pdbl x y id | pmadd x1 y1 id1 x2 y2        -> x y id
//   jdbl X Y Z                    -> x y id    (the double of a Jacobian point given as it is: how a point with Y = 0 gets in)
//   pmul k x y                    -> x y id    (k: 256 bits in the low 64 hex digits)
//   subgroup r x y                -> flag      ([r] P = identity; the first operand is ignored)
//   dec96 xw yw                   -> class x y (class 0 identity, 1 point, 2 malformed; the words as read from the wire)
//   dec48 cw                      -> class x y
//   enc id x y                    -> xw yw cw  (both encodings of a point)
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>
#include <string>
#include <vector>

#include "../../ecsimd_amd/csrc/g1.cuh"

using namespace ecsimd_hip;

static fe381 parse(const char* s) {
  fe381 r;
  for (int j = 0; j < 12; ++j) { unsigned v = 0; sscanf(s + 8 * j, "%8x", &v); r.w[11 - j] = v; }
  return r;
}
static void show(const fe381& a) {
  for (int j = 11; j >= 0; --j) printf("%08x", a.w[j]);
  printf(" ");
}
static void show_flag(bool f) { show(fe384_small(f ? 1u : 0u)); }
static void show_plain(const fe381& a) { show(fe381_from_mont(a)); }
static void show_point(const g1_point& p) {
  if (g1_is_identity(p)) { show(fe381_zero()); show(fe381_zero()); show_flag(true); return; }
  const g1_affine a = g1_to_affine(p);
  show_plain(a.x); show_plain(a.y); show_flag(false);
}
static g1_point point_of(const fe381& x, const fe381& y, const fe381& id) {
  return id.w[0] ? g1_identity() : g1_from_affine({fe381_to_mont(x), fe381_to_mont(y)});
}

int main() {
  static char line[4096];
  while (fgets(line, sizeof line, stdin)) {
    std::vector<fe381> a;
    char* tok = strtok(line, " \n");
    if (!tok) continue;
    const std::string op = tok;
    while ((tok = strtok(nullptr, " \n"))) a.push_back(parse(tok));
    if (op == "mul") show_plain(fe381_mul(fe381_to_mont(a[0]), fe381_to_mont(a[1])));
    else if (op == "sqr") show_plain(fe381_sqr(fe381_to_mont(a[0])));
    else if (op == "add") show_plain(fe381_add(fe381_to_mont(a[0]), fe381_to_mont(a[1])));
    else if (op == "sub") show_plain(fe381_sub(fe381_to_mont(a[0]), fe381_to_mont(a[1])));
    else if (op == "neg") show_plain(fe381_neg(fe381_to_mont(a[0])));
    else if (op == "inv") show_plain(fe381_invert(fe381_to_mont(a[0])));
    else if (op == "canon") show_plain(fe381_to_mont(a[0]));
    else if (op == "sqrt") { bool ok; const fe381 s = fe381_sqrt(fe381_to_mont(a[0]), ok); show_plain(s); show_flag(ok); }
    else if (op == "lex") show_flag(fe381_lex_largest(fe381_to_mont(a[0])));
    else if (op == "padd") show_point(g1_add(point_of(a[0], a[1], a[2]), point_of(a[3], a[4], a[5])));
    else if (op == "pdbl") show_point(g1_dbl(point_of(a[0], a[1], a[2])));
    else if (op == "pmadd") show_point(g1_madd(point_of(a[0], a[1], a[2]), fe381_to_mont(a[3]), fe381_to_mont(a[4])));
    else if (op == "jdbl") { g1_point p; p.x = fe381_to_mont(a[0]); p.y = fe381_to_mont(a[1]); p.z = fe381_to_mont(a[2]); show_point(g1_dbl(p)); }
    else if (op == "pmul") {
      uint32_t k[8];
      for (int q = 0; q < 8; ++q) k[q] = a[0].w[q];
      show_point(g1_mul(k, {fe381_to_mont(a[1]), fe381_to_mont(a[2])}));
    } else if (op == "subgroup") show_flag(g1_in_subgroup({fe381_to_mont(a[1]), fe381_to_mont(a[2])}));
    else if (op == "dec96") { g1_affine p; const int cls = g1_decode96(a[0], a[1], p); show(fe384_small((uint32_t)cls)); show_plain(p.x); show_plain(p.y); }
    else if (op == "dec48") { g1_affine p; const int cls = g1_decode48(a[0], p); show(fe384_small((uint32_t)cls)); show_plain(p.x); show_plain(p.y); }
    else if (op == "enc") {
      const int cls = a[0].w[0] ? G1_INFINITY : G1_POINT;
      const g1_affine p = {fe381_to_mont(a[1]), fe381_to_mont(a[2])};
      fe381 xw, yw;
      g1_encode96(cls, p, xw, yw);
      show(xw); show(yw); show(g1_encode48(cls, p));
    } else { fprintf(stderr, "unknown op %s\n", op.c_str()); return 2; }
    printf("\n");
  }
  return 0;
}
