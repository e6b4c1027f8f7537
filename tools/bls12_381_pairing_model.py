#!/usr/bin/env python3
"""bls12_381_pairing_model.py -- the optimal ate pairing of BLS12-381 as Python integers: THE DEFINITION a device pairing is held to.

Deliberately the slow textbook form, so that device code (a Karatsuba tower, projective lines on the twist, chains by x) shares no algorithm with it:
  FIELD     Fp12 = Fp[w] / (w^12 - 2 w^6 + 2), twelve coefficients, schoolbook products, the inverse by the extended Euclidean algorithm on polynomials.  The
            tower Fp2[v] / (v^3 - (1 + u)), Fp6[w] / (w^2 - v) embeds by v = w^2, u = w^6 - 1 (to_poly / to_tower).
  UNTWIST   a point (x', y') of E' maps to (x' / w^2, y' / w^3) on E: y^2 = x^3 + 4 over Fp12.
  MILLER    affine chord and tangent lines over Fp12 evaluated at P, the point arithmetic on E(Fp12) itself, over the bits of |x| = 0xd201000000010000.
  SIGN      x is negative: the loop's value is conjugated (w -> -w, the p^6 power).
  EXPONENT  e(P, Q) = that value to the power (p^12 - 1) / r by ONE plain square-and-multiply.
  IDENTITY  e(infinity, Q) = e(P, infinity) = 1.
No published vector pins the value (nothing could be fetched where this was written): the definition above and the algebraic checks of _self_check do.

GT ON THE WIRE (ours: there is no standard): 576 bytes, twelve 48-byte big-endian canonical residues in TOWER order, the coefficient of u^k v^j w^i at index
6 i + 2 j + k.

    python3 tools/bls12_381_pairing_model.py            writes tests/golden/bls12_381_pairing_vectors.json (about half a minute)
"""
import json
import os
import random
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bls12_381_model as g1                                          # noqa: E402
import bls12_381_g2_model as g2                                       # noqa: E402
from bls12_381_model import P, R, X                                   # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "bls12_381_pairing_vectors.json")
ABS_X = -X
FULL_EXPONENT = (P ** 12 - 1) // R
HARD_EXPONENT = (P ** 4 - P ** 2 + 1) // R
ONE = (1,) + (0,) * 11
ZERO = (0,) * 12
W = (0, 1) + (0,) * 10


# ---- Fp12 as polynomials in w of degree below 12, lowest coefficient first
def _reduce(c):
    c = list(c)
    for d in range(len(c) - 1, 11, -1):                               # w^12 = 2 w^6 - 2
        t = c[d]
        c[d - 6] += 2 * t
        c[d - 12] -= 2 * t
    return tuple(v % P for v in c[:12])


def f12_mul(a, b):
    c = [0] * 23
    for i, x in enumerate(a):
        if x:
            for j, y in enumerate(b):
                c[i + j] += x * y
    return _reduce(c)


def f12_add(a, b):
    return tuple((x + y) % P for x, y in zip(a, b))


def f12_sub(a, b):
    return tuple((x - y) % P for x, y in zip(a, b))


def f12_neg(a):
    return tuple(-x % P for x in a)


def f12_scalar(a, s):
    return tuple(x * s % P for x in a)


def f12_pow(a, e):
    r = ONE
    for bit in bin(e)[2:]:
        r = f12_mul(r, r)
        if bit == "1":
            r = f12_mul(r, a)
    return r


def _poly_divmod(a, b):
    """(quotient, remainder) of polynomials over Fp; b's leading coefficient is non-zero."""
    a = list(a)
    inv = pow(b[-1], -1, P)
    q = [0] * max(1, len(a) - len(b) + 1)
    for d in range(len(a) - len(b), -1, -1):
        t = a[d + len(b) - 1] * inv % P
        q[d] = t
        for i, y in enumerate(b):
            a[d + i] = (a[d + i] - t * y) % P
    rem = a[:len(b) - 1]
    while rem and rem[-1] == 0:
        rem.pop()
    return q, rem


def _poly_mul(a, b):
    c = [0] * (len(a) + len(b) - 1) if a and b else []
    for i, x in enumerate(a):
        for j, y in enumerate(b):
            c[i + j] = (c[i + j] + x * y) % P
    return c


def _poly_sub(a, b):
    n = max(len(a), len(b))
    c = [((a[i] if i < len(a) else 0) - (b[i] if i < len(b) else 0)) % P for i in range(n)]
    while c and c[-1] == 0:
        c.pop()
    return c


def f12_inv(a):
    """1 / a by the extended Euclidean algorithm against w^12 - 2 w^6 + 2; 0 -> 0 (the rule fp2.cuh's inverse has)."""
    r1 = [v % P for v in a]
    while r1 and r1[-1] == 0:
        r1.pop()
    if not r1:
        return ZERO
    r0 = [2, 0, 0, 0, 0, 0, P - 2, 0, 0, 0, 0, 0, 1]
    t0, t1 = [], [1]
    while len(r1) > 1:
        q, rem = _poly_divmod(r0, r1)
        r0, r1 = r1, rem
        t0, t1 = t1, _poly_sub(t0, _poly_mul(q, t1))
    assert len(r1) == 1                                              # the modulus is irreducible: the gcd is a constant
    s = pow(r1[0], -1, P)
    out = [v * s % P for v in t1]
    return _reduce(out + [0] * (12 - len(out)))


def f12_conj(a):
    """w -> -w: the automorphism of Fp12 over Fp6, which is the p^6 power."""
    return tuple(-x % P if i & 1 else x % P for i, x in enumerate(a))


def f12_frobenius(a, k=1):
    """a^(p^k), by plain exponentiation."""
    return f12_pow(a, P ** k)


def cyclotomic(f):
    """f^((p^6 - 1)(p^2 + 1)): a member of the cyclotomic subgroup (where the inverse is the conjugate)."""
    return f12_pow(f, (P ** 6 - 1) * (P ** 2 + 1))


# ---- the tower <-> the polynomial.  Tower index 6 i + 2 j + k holds the coefficient of u^k v^j w^i; u^k v^j w^i = (w^6 - 1)^k w^(2 j + i).
def to_poly(t):
    a = [0] * 12
    for i in range(2):
        for j in range(3):
            c0, c1 = t[6 * i + 2 * j], t[6 * i + 2 * j + 1]
            e = 2 * j + i
            a[e] = (c0 - c1) % P
            a[e + 6] = c1 % P
    return tuple(a)


def to_tower(a):
    t = [0] * 12
    for e in range(6):
        i, j = e & 1, e >> 1
        t[6 * i + 2 * j] = (a[e] + a[e + 6]) % P
        t[6 * i + 2 * j + 1] = a[e + 6] % P
    return tuple(t)


def fp2_in_f12(c):
    """The element c0 + c1 u of Fp2 inside Fp12: u = w^6 - 1."""
    a = [0] * 12
    a[0], a[6] = (c[0] - c[1]) % P, c[1] % P
    return tuple(a)


def tower_mul(a, b):
    return to_tower(f12_mul(to_poly(a), to_poly(b)))


def f6_to_f12(t6):
    """Six tower coefficients (index 2 j + k) as the element of Fp6 inside Fp12."""
    return to_poly(tuple(t6) + (0,) * 6)


def gt_encode(a):
    return b"".join(v.to_bytes(48, "big") for v in to_tower(a))


def gt_decode(b):
    assert len(b) == 576
    t = tuple(int.from_bytes(b[48 * i:48 * i + 48], "big") for i in range(12))
    assert max(t) < P
    return to_poly(t)


# ---- E: y^2 = x^3 + 4 over Fp12, affine, None the identity
W_INV = f12_inv(W)
W2_INV = f12_mul(W_INV, W_INV)
W3_INV = f12_mul(W2_INV, W_INV)


def untwist(q):
    return None if q is None else (f12_mul(fp2_in_f12(q[0]), W2_INV), f12_mul(fp2_in_f12(q[1]), W3_INV))


def embed(p):
    return None if p is None else ((p[0] % P,) + (0,) * 11, (p[1] % P,) + (0,) * 11)


def e12_on_curve(pt):
    x, y = pt
    return f12_mul(y, y) == f12_add(f12_mul(f12_mul(x, x), x), (4,) + (0,) * 11)


def _line_and_sum(t, q, at):
    """(the line through t and q -- the tangent where t = q -- evaluated at `at`, t + q).  Neither point is the identity and t != -q: r is prime and larger
    than |x|, so the loop never meets those cases on members of the groups."""
    (x1, y1), (x2, y2) = t, q
    if t == q:
        lam = f12_mul(f12_scalar(f12_mul(x1, x1), 3), f12_inv(f12_scalar(y1, 2)))
    else:
        assert x1 != x2
        lam = f12_mul(f12_sub(y2, y1), f12_inv(f12_sub(x2, x1)))
    x3 = f12_sub(f12_sub(f12_mul(lam, lam), x1), x2)
    y3 = f12_sub(f12_mul(lam, f12_sub(x1, x3)), y1)
    line = f12_sub(f12_sub(at[1], y1), f12_mul(lam, f12_sub(at[0], x1)))
    return line, (x3, y3)


def miller(p, q):
    """f_{|x|, Q}(P), conjugated for the sign of x; p a point of E(Fp), q a point of E'(Fp2); 1 where either is the identity."""
    if p is None or q is None:
        return ONE
    at, base = embed(p), untwist(q)
    f, t = ONE, base
    for bit in bin(ABS_X)[3:]:
        line, t = _line_and_sum(t, t, at)
        f = f12_mul(f12_mul(f, f), line)
        if bit == "1":
            line, t = _line_and_sum(t, base, at)
            f = f12_mul(f, line)
    return f12_conj(f)


def final_exp(f):
    return f12_pow(f, FULL_EXPONENT)


def pairing(p, q):
    return final_exp(miller(p, q))


# ---- the facts the device code relies on
def _identities():
    assert f12_mul(W, W_INV) == ONE
    u = f12_sub(f12_pow(W, 6), ONE)
    assert f12_mul(u, u) == f12_neg(ONE)                             # u^2 = -1
    v = f12_mul(W, W)
    assert f12_mul(f12_mul(v, v), v) == f12_add(ONE, u)              # v^3 = 1 + u
    assert to_poly(to_tower(tuple(range(1, 13)))) == tuple(range(1, 13)) and to_tower(u) == (0, 1) + (0,) * 10
    assert (X - 1) % 3 == 0 and (ABS_X + 1) % 3 == 0
    assert HARD_EXPONENT * R == P ** 4 - P ** 2 + 1
    assert HARD_EXPONENT == ((X - 1) ** 2 // 3) * (X + P) * (X * X + P * P - 1) + 1
    assert FULL_EXPONENT == (P ** 6 - 1) * (P ** 2 + 1) * HARD_EXPONENT
    assert R % 3 != 0                                                 # so the cube of a value of order dividing r is 1 only where the value is
    assert ((ABS_X + 1) ** 2 // 3).bit_length() == 126 and bin((ABS_X + 1) ** 2 // 3).count("1") == 48


_identities()


def _self_check(gt=None):
    """The slow part (several pairings): non-degeneracy, the order, bilinearity in both arguments separately."""
    gt = pairing(g1.G, g2.G) if gt is None else gt
    assert e12_on_curve(untwist(g2.G)) and e12_on_curve(embed(g1.G))
    assert gt != ONE and f12_pow(gt, R) == ONE
    a, b = 0x1234567, 0x89abcde
    assert pairing(g1.mul(a, g1.G), g2.G) == f12_pow(gt, a)
    assert pairing(g1.G, g2.mul(b, g2.G)) == f12_pow(gt, b)
    assert pairing(None, g2.G) == ONE and pairing(g1.G, None) == ONE
    c = cyclotomic(tuple(range(3, 15)))
    assert f12_mul(c, f12_conj(c)) == ONE
    return gt


# ---- the fixture
def _hx(t):
    return ["%096x" % v for v in t]


def tower_operands():
    """Fp12 operands in tower order on the representation's bounds, and with zeros in every sparse position."""
    rng = random.Random(381212)
    rnd = lambda: tuple(rng.randrange(P) for _ in range(12))
    ops = [tuple([0] * 12), tuple([1] + [0] * 11), tuple([P - 1] * 12), tuple([P - 1] + [0] * 11), tuple([0] * 11 + [P - 1]), tuple([1] * 12)]
    for keep in ((0, 1), (2, 3), (4, 5), (6, 7), (8, 9), (10, 11), (0, 1, 2, 3, 8, 9), (0, 1, 2, 3, 4, 5), (6, 7, 8, 9, 10, 11)):
        r = rnd()
        ops.append(tuple(r[i] if i in keep else 0 for i in range(12)))
    ops += [rnd() for _ in range(4)]
    return ops


def build_fixture():
    f1 = json.load(open(g1.FIXTURE))
    f2 = json.load(open(g2.FIXTURE))
    gt = _self_check()
    p_of = lambda i: g1.decode96(bytes.fromhex(f1["multiples"][i]["uncompressed"]))
    q_of = lambda i: g2.decode192(bytes.fromhex(f2["multiples"][i]["uncompressed"]))
    pairs = []
    for i, j in ((1, 1), (12, 13), (9, 11), (14, 2), (0, 12), (13, 0), (0, 0)):
        p, q = p_of(i), q_of(j)
        val = gt if (i, j) == (1, 1) else pairing(p, q)
        a, b = int(f1["multiples"][i]["k"], 16), int(f2["multiples"][j]["k"], 16)
        assert val == f12_pow(gt, a * b % R)                         # bilinearity on every record
        pairs.append(dict(g1=g1.encode96(p).hex(), g2=g2.encode192(q).hex(), a="%x" % a, b="%x" % b, gt=gt_encode(val).hex()))
    rng = random.Random(12381)
    cyc = [cyclotomic(tuple(rng.randrange(P) for _ in range(12))) for _ in range(2)] + [gt]
    for c in cyc:
        assert f12_mul(c, f12_conj(c)) == ONE
    return {
        "about": "tools/bls12_381_pairing_model.py: the BLS12-381 pairing; a Gt value is 576 bytes, twelve big-endian residues in tower order (u^k v^j w^i at 6i+2j+k)",
        "generators": gt_encode(gt).hex(),
        "pairings": pairs,
        "tower_operands": [_hx(t) for t in tower_operands()],
        "cyclotomic": [_hx(to_tower(c)) for c in cyc],
        "malformed_g1": [m["bytes"] for m in f1["malformed_uncompressed"]],
        "malformed_g2": [m["bytes"] for m in f2["malformed_uncompressed"]],
        "off_subgroup_g1": [m["uncompressed"] for m in f1["off_subgroup"]],
        "off_subgroup_g2": [m["uncompressed"] for m in f2["off_subgroup"]],
    }


def fixture_text():
    return json.dumps(build_fixture(), indent=1, sort_keys=True) + "\n"


if __name__ == "__main__":
    with open(FIXTURE, "w") as f:
        f.write(fixture_text())
    print(FIXTURE, file=sys.stderr)
