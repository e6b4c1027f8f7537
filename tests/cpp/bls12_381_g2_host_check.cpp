// bls12_381_g2_host_check.cpp -- fp2.cuh / g2.cuh on the HOST: the extension field, the group law with its branches, the scalar product, the subgroup test and
// the serialisation's rules as the kernels run them.  tests/test_bls12_381_g2_cpu.py feeds it operands and compares the answers with Python integers and
// tools/bls12_381_g2_model.py.  No GPU is involved: the logic is right before a device runs it.
//
// stdin: one request per line, "<op> <96 hex digits> ..."; stdout: the results as 96 hex digits each, space-separated.  An Fp2 operand is TWO records, c0 then
// c1, each ANY 384-bit value; a point is x, y (four records) and a flag record.
//   mul a b | sqr a | add a b | sub a b | neg a | conj a | dbl a | inv a | canon a   -> the plain residues c0 c1
//   iszero a | eq a b | lex a     -> flag
//   sqrt a                        -> c0 c1 flag (the candidate and "its square is a")
//   padd P Q | pdbl P | pmadd P x2 y2           -> x y id   (id = 1: the identity, coordinates ignored; points are NOT validated)
//   jdbl X Y Z                    -> x y id    (the double of a Jacobian point given as it is: how a point with Y = 0 gets in)
//   pmul k x y                    -> x y id    (k: 256 bits in the low 64 hex digits)
//   subgroup x y                  -> flag      ([r] Q = identity)
//   dec192 x1w x0w y1w y0w        -> class x y (class 0 identity, 1 point, 2 malformed; the words as read from the wire, c1 first)
//   dec96 c1w c0w                 -> class x y
//   enc id x y                    -> x1w x0w y1w y0w c1w c0w  (both encodings of a point, in wire order)
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>
#include <string>
#include <vector>

#include "../../ecsimd_amd/csrc/g2.cuh"

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
static void show2(const fp2& a) { show(fe381_from_mont(a.c0)); show(fe381_from_mont(a.c1)); }
static void show_point(const g2_point& p) {
  if (g2_is_identity(p)) { show2(fp2_zero()); show2(fp2_zero()); show_flag(true); return; }
  const g2_affine a = g2_to_affine(p);
  show2(a.x); show2(a.y); show_flag(false);
}

int main() {
  static char line[8192];
  while (fgets(line, sizeof line, stdin)) {
    std::vector<fe381> a;
    char* tok = strtok(line, " \n");
    if (!tok) continue;
    const std::string op = tok;
    while ((tok = strtok(nullptr, " \n"))) a.push_back(parse(tok));
    const auto el = [&](size_t j) { return fp2_to_mont(a[j], a[j + 1]); };                  // the Fp2 operand at records j, j + 1
    const auto pt = [&](size_t j) { return a[j + 4].w[0] ? g2_identity() : g2_from_affine({el(j), el(j + 2)}); };   // the point at records j .. j + 4
    if (op == "mul") show2(fp2_mul(el(0), el(2)));
    else if (op == "sqr") show2(fp2_sqr(el(0)));
    else if (op == "add") show2(fp2_add(el(0), el(2)));
    else if (op == "sub") show2(fp2_sub(el(0), el(2)));
    else if (op == "neg") show2(fp2_neg(el(0)));
    else if (op == "conj") show2(fp2_conj(el(0)));
    else if (op == "dbl") show2(fp2_dbl(el(0)));
    else if (op == "inv") show2(fp2_invert(el(0)));
    else if (op == "canon") show2(el(0));
    else if (op == "iszero") show_flag(fp2_is_zero(el(0)));
    else if (op == "eq") show_flag(fp2_equal(el(0), el(2)));
    else if (op == "lex") show_flag(fp2_lex_largest(el(0)));
    else if (op == "sqrt") { bool ok; const fp2 s = fp2_sqrt(el(0), ok); show2(s); show_flag(ok); }
    else if (op == "padd") show_point(g2_add(pt(0), pt(5)));
    else if (op == "pdbl") show_point(g2_dbl(pt(0)));
    else if (op == "pmadd") show_point(g2_madd(pt(0), {el(5), el(7)}));
    else if (op == "jdbl") { g2_point p; p.x = el(0); p.y = el(2); p.z = el(4); show_point(g2_dbl(p)); }
    else if (op == "pmul") {
      uint32_t k[8];
      for (int q = 0; q < 8; ++q) k[q] = a[0].w[q];
      show_point(g2_mul(k, {el(1), el(3)}));
    } else if (op == "subgroup") show_flag(g2_in_subgroup({el(0), el(2)}));
    else if (op == "dec192") { g2_affine p; const int cls = g2_decode192(a[0], a[1], a[2], a[3], p); show(fe384_small((uint32_t)cls)); show2(p.x); show2(p.y); }
    else if (op == "dec96") { g2_affine p; const int cls = g2_decode96(a[0], a[1], p); show(fe384_small((uint32_t)cls)); show2(p.x); show2(p.y); }
    else if (op == "enc") {
      const int cls = a[0].w[0] ? G2_INFINITY : G2_POINT;
      const g2_affine p = {el(1), el(3)};
      fe381 w[6];
      g2_encode192(cls, p, w[0], w[1], w[2], w[3]);
      g2_encode96(cls, p, w[4], w[5]);
      for (int j = 0; j < 6; ++j) show(w[j]);
    } else { fprintf(stderr, "unknown op %s\n", op.c_str()); return 2; }
    printf("\n");
  }
  return 0;
}
