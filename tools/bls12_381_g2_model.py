#!/usr/bin/env python3
"""bls12_381_g2_model.py -- BLS12-381 G2 as Python integers: THE DEFINITION behind include/ecsimd_bls12_381_g2.h.

Fp2 = Fp[u] / (u^2 + 1) as pairs (c0, c1), the affine textbook group law on E': y^2 = x^3 + 4 (1 + u), the ZCash / IETF serialisation (192 bytes
uncompressed, 96 compressed, c1 BEFORE c0), the subgroup test as [r]Q = infinity with the psi form as a second opinion, the multi-scalar multiplication as a
plain sum, and the schedule ecsimd_bls381_g2_msm_plan reports.  p, r, x and the bucket schedule come from bls12_381_model.py; none of the library's code.  At
import the curve facts the device code relies on are asserted.

    python3 tools/bls12_381_g2_model.py            writes tests/golden/bls12_381_g2_vectors.json
"""
import json
import os
import random
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bls12_381_model import P, R, X, plan as g1_plan, fe_sqrt, is_prime, _tree_passes      # noqa: E402
from bls12_381_model import MSM_MAX_N, ALG_AUTO, ALG_BUCKETS, ALG_LANES, TREE_FAN, MONT_R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "bls12_381_g2_vectors.json")

H2 = 0x5d543a95414e7f1091d50792876a202cd91de4547085abaa68a205b2e5a7ddfa628f1cb4d9e82ef21537e293a6691ae1616ec6e786f0c70cf1c38e31c7238e5
B2 = (4, 4)                                                          # 4 (1 + u)
GX = (0x024aa2b2f08f0a91260805272dc51051c6e47ad4fa403b02b4510b647ae3d1770bac0326a805bbefd48056c8c121bdb8,
      0x13e02b6052719f607dacd3a088274f65596bd0d09920b61ab5da61bbdc7f5049334cf11213945d57e5ac7d055d042b7e)
GY = (0x0ce5d527727d6e118cc9cdc6da2e351aadfd9baa8cbdd3a76d429a695160d12c923ac9cc3baca289e193548608b82801,
      0x0606c4a02ea734cc32acd2b02bc28b99cb3e287e85a763af267492ab572e99ab3f370d275cec1da1aaa9075ff05f79be)
G = (GX, GY)
INF = None
HALF = (P - 1) // 2
ELEM = 96


# ---- Fp2: pairs of integers below p
def f2(a):
    return (a[0] % P, a[1] % P)


def f2_add(a, b):
    return ((a[0] + b[0]) % P, (a[1] + b[1]) % P)


def f2_sub(a, b):
    return ((a[0] - b[0]) % P, (a[1] - b[1]) % P)


def f2_neg(a):
    return (-a[0] % P, -a[1] % P)


def f2_mul(a, b):
    return ((a[0] * b[0] - a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)


def f2_sqr(a):
    return f2_mul(a, a)


def f2_conj(a):
    return (a[0] % P, -a[1] % P)


def f2_inv(a):
    """1 / a; 0 -> 0 (the device's rule)."""
    n = pow((a[0] * a[0] + a[1] * a[1]) % P, P - 2, P)
    return (a[0] * n % P, -a[1] * n % P)


def f2_pow(a, e):
    r, a = (1, 0), f2(a)
    while e:
        if e & 1:
            r = f2_mul(r, a)
        a = f2_sqr(a)
        e >>= 1
    return r


def f2_sqrt(a):
    """A square root of a in Fp2, or None: the p = 3 mod 4 algorithm on Fp2 exponentiations (not the device's route through the norm)."""
    a = f2(a)
    if a == (0, 0):
        return (0, 0)
    a1 = f2_pow(a, (P - 3) // 4)
    alpha = f2_mul(f2_sqr(a1), a)
    x0 = f2_mul(a1, a)
    if f2_mul(f2_conj(alpha), alpha) == (P - 1, 0):
        return None
    if alpha == (P - 1, 0):
        s = f2_mul((0, 1), x0)                                       # the alpha = -1 branch
    else:
        s = f2_mul(f2_pow(f2_add((1, 0), alpha), (P - 1) // 2), x0)
    return s if f2_sqr(s) == a else None


def lex_largest(y):
    y = f2(y)
    return y[1] > HALF or (y[1] == 0 and y[0] > HALF)


# ---- the group: affine points (x, y) of pairs, INF = None
def on_curve(pt):
    if pt is INF:
        return True
    x, y = pt
    return all(0 <= v < P for v in x + y) and f2_sqr(y) == f2_add(f2_mul(f2_sqr(x), x), B2)


def neg(pt):
    return INF if pt is INF else (pt[0], f2_neg(pt[1]))


def add(p1, p2):
    if p1 is INF:
        return p2
    if p2 is INF:
        return p1
    x1, y1 = p1
    x2, y2 = p2
    if x1 == x2:
        if f2_add(y1, y2) == (0, 0):
            return INF                                               # P + (-P), and the double of a point with y = 0
        lam = f2_mul(f2_mul((3, 0), f2_sqr(x1)), f2_inv(f2_add(y1, y1)))
    else:
        lam = f2_mul(f2_sub(y2, y1), f2_inv(f2_sub(x2, x1)))
    x3 = f2_sub(f2_sub(f2_sqr(lam), x1), x2)
    return (x3, f2_sub(f2_mul(lam, f2_sub(x1, x3)), y1))


def mul(k, pt):
    """k Q for an integer k >= 0: the sum is over the integers, so Q need not lie in G2."""
    acc = INF
    while k:
        if k & 1:
            acc = add(acc, pt)
        pt = add(pt, pt)
        k >>= 1
    return acc


def in_subgroup(pt):
    return mul(R, pt) is INF


PSI_X = f2_inv(f2_pow((1, 1), (P - 1) // 3))
PSI_Y = f2_inv(f2_pow((1, 1), (P - 1) // 2))


def psi(pt):
    return INF if pt is INF else (f2_mul(f2_conj(pt[0]), PSI_X), f2_mul(f2_conj(pt[1]), PSI_Y))


def psi_in_subgroup(pt):
    """psi(Q) = [x] Q (x < 0: -[|x|] Q): the test that costs a 64-bit product; g2_check ships the definition, this is the second opinion."""
    return psi(pt) == neg(mul(-X, pt))


def msm(scalars, points, bits=256):
    acc = INF
    for k, pt in zip(scalars, points):
        acc = add(acc, mul(k % (1 << bits), pt))
    return acc


# ---- the encodings: c1 before c0
def b48(v):
    return v.to_bytes(48, "big")


def encode192(pt):
    if pt is INF:
        return b"\x40" + bytes(191)
    (x0, x1), (y0, y1) = pt
    return b48(x1) + b48(x0) + b48(y1) + b48(y0)


def encode96(pt):
    if pt is INF:
        return b"\xc0" + bytes(95)
    b = bytearray(b48(pt[0][1]) + b48(pt[0][0]))
    b[0] |= 0x80 | (0x20 if lex_largest(pt[1]) else 0)
    return bytes(b)


MALFORMED = "malformed"


def decode192(b):
    """The point, INF, or MALFORMED.  On-curve only: no subgroup test."""
    assert len(b) == 192
    flags = b[0] & 0xe0
    if flags == 0x40:
        return INF if b == b"\x40" + bytes(191) else MALFORMED
    if flags != 0:
        return MALFORMED
    x1, x0, y1, y0 = (int.from_bytes(b[48 * j:48 * j + 48], "big") for j in range(4))
    if max(x1, x0, y1, y0) >= P:
        return MALFORMED
    pt = ((x0, x1), (y0, y1))
    return pt if on_curve(pt) else MALFORMED


def decode96(b):
    assert len(b) == 96
    if not b[0] & 0x80:
        return MALFORMED
    if b[0] & 0x40:
        return INF if b == b"\xc0" + bytes(95) else MALFORMED
    x1 = int.from_bytes(bytes([b[0] & 0x1f]) + b[1:48], "big")
    x0 = int.from_bytes(b[48:], "big")
    if x1 >= P or x0 >= P:
        return MALFORMED
    x = (x0, x1)
    y = f2_sqrt(f2_add(f2_mul(f2_sqr(x), x), B2))
    if y is None:
        return MALFORMED
    if lex_largest(y) != bool(b[0] & 0x20):
        y = f2_neg(y)
    return (x, y)


# ---- the schedule (ecsimd_bls381_g2_msm_plan: capi.hip g2_schedule_of): the G1 model's bucket schedule with 96-byte elements; LANES is 16 + 288 n bytes
def plan(n, bits, flags, threshold):
    if not (1 <= bits <= 256) or n > MSM_MAX_N or flags not in (ALG_AUTO, ALG_BUCKETS, ALG_LANES):
        return None
    route = flags if flags != ALG_AUTO else (ALG_BUCKETS if n >= threshold else ALG_LANES)
    if n == 0 or route == ALG_BUCKETS:
        out = g1_plan(n, bits, ALG_BUCKETS, threshold, elem=ELEM, planes=3)
        out["route"] = route
        return out
    return dict(route=ALG_LANES, c=0, windows=0, buckets=0, L=0, m=0, max_chain=TREE_FAN, launches=3 + _tree_passes(n), workspace_bytes=16 + 3 * ELEM * n)


# ---- the fixture's points
def curve_point(x0, x1=0):
    """The first point of E' with x = (x0 + j, x1), j >= 0, and the y that is NOT the lexicographically largest."""
    while True:
        x = (x0 % P, x1 % P)
        y = f2_sqrt(f2_add(f2_mul(f2_sqr(x), x), B2))
        if y is not None:
            return (x, f2_neg(y) if lex_largest(y) else y)
        x0 += 1


def off_subgroup_points(count=4):
    pts, x0 = [], 1
    while len(pts) < count:
        pt = curve_point(x0, len(pts))                               # x.c1 = 0, 1, 2, 3
        x0 = pt[0][0] + 1
        if not in_subgroup(pt):
            pts.append(pt if len(pts) % 2 == 0 else neg(pt))
    return pts


def h_torsion_point():
    """[r] Q for a point Q of E'(Fp2): order dividing h2, not the identity, so outside G2."""
    x0 = 1
    while True:
        q = curve_point(x0, 7)
        t = mul(R, q)
        if t is not INF:
            return t
        x0 = q[0][0] + 1


def cofactor_cleared_point():
    """[h2] Q for a point Q of E'(Fp2): in G2."""
    x0 = 1
    while True:
        q = curve_point(x0, 11)
        t = mul(H2, q)
        if t is not INF:
            return t
        x0 = q[0][0] + 1


def real_and_imaginary_y_points():
    """(a point with y.c1 = 0, a point with y.c0 = 0): x = (x0, x1) with 3 x0^2 x1 - x1^3 = -4 makes x^3 + 4 (1 + u) an element v of Fp; y is the real
    sqrt(v) where v is a residue and u sqrt(-v) where it is not.  The first x1 = 1, 2, ... of each kind, the smaller x0."""
    real = imag = None
    x1 = 1
    while real is None or imag is None:
        x0 = fe_sqrt((x1 ** 3 - 4) * pow(3 * x1, -1, P))
        if x0 is not None:
            x0 = min(x0, P - x0)
            x = (x0, x1)
            rhs = f2_add(f2_mul(f2_sqr(x), x), B2)
            assert rhs[1] == 0
            y = f2_sqrt(rhs)
            if y[1] == 0 and real is None:
                real = (x, (min(y[0], P - y[0]), 0))
            if y[0] == 0 and imag is None:
                imag = (x, (0, min(y[1], P - y[1])))
        x1 += 1
    return real, imag


# ---- the curve facts, asserted at import
def _self_check(records=()):
    assert f2_mul((0, 1), (0, 1)) == (P - 1, 0) and P % 4 == 3       # u^2 = -1, and -1 is no square of Fp
    assert H2 == (X ** 8 - 4 * X ** 7 + 5 * X ** 6 - 4 * X ** 4 + 6 * X ** 3 - 4 * X ** 2 - 4 * X + 13) // 9
    assert (X ** 8 - 4 * X ** 7 + 5 * X ** 6 - 4 * X ** 4 + 6 * X ** 3 - 4 * X ** 2 - 4 * X + 13) % 9 == 0 and H2.bit_length() == 507 and H2 % 2 == 1
    assert is_prime(P) and is_prime(R)
    assert on_curve(G) and mul(R, G) is INF and in_subgroup(G) and psi_in_subgroup(G)
    enc = encode96(G)
    assert enc[0] == 0x93 and enc[1:48] == b48(GX[1])[1:] and enc[48:] == b48(GX[0]) and decode96(enc) == G and decode192(encode192(G)) == G
    b4 = 0x09d645513d83de7e8ec9733bbf78ab2fb1d37ebee6ba24d7478fe97a6b0a807f53cc0032fc34000aaa270000000cfff3
    assert 4 * MONT_R % P == b4 and B2 == (4, 4)                     # in Montgomery form both components of b' are fe381.cuh's B4
    assert f2_sqrt((4, 0)) in ((2, 0), (P - 2, 0))                   # a residue of Fp: a real root
    assert f2_sqrt((P - 4, 0)) in ((0, 2), (0, P - 2))               # a non-residue of Fp: a purely imaginary root
    assert f2_sqrt((1, 1)) is None or f2_sqr(f2_sqrt((1, 1))) == (1, 1)
    q = curve_point(1, 5)
    assert on_curve(q) and mul(H2 * R, q) is INF                     # the curve's order kills every point of E'(Fp2)
    assert not in_subgroup(q) and not psi_in_subgroup(q)             # psi(Q) = [x] Q fails outside G2
    assert in_subgroup(mul(H2, q)) and psi_in_subgroup(mul(H2, q))
    for r in records:                                                # psi against the definition on a fixture's records
        pt = decode192(bytes.fromhex(r["uncompressed"]))
        assert pt is not MALFORMED and in_subgroup(pt) == psi_in_subgroup(pt) == r["in_subgroup"]


_self_check()


def field_operands():
    """The representation's bounds (fe381.cuh: every 384-bit value is accepted at the door, everything inside is canonical); Fp2 operands are pairs of them."""
    top = (1 << 384) - 1
    return [0, 1, 2, P - 2, P - 1, P, P + 1, 9 * P + 1, top - 1, top, MONT_R % P, HALF, HALF + 1, 1 << 383,
            int.from_bytes(b"\xff\xff\xff\xff\x00\x00\x00\x00" * 6, "big")]


def malformed_records():
    g = [b48(GX[1]), b48(GX[0]), b48(GY[1]), b48(GY[0])]             # wire order
    join = lambda parts: b"".join(parts)
    swap = lambda j, v: join(g[:j] + [v] + g[j + 1:])
    no_root = next(x0 for x0 in range(1, 100) if f2_sqrt(f2_add(f2_mul(f2_sqr((x0, 0)), (x0, 0)), B2)) is None)
    names = ("x.c1", "x.c0", "y.c1", "y.c0")
    u, c = [], []
    for j in range(4):
        u.append((names[j] + " is p", swap(j, b48(P))))
        u.append((names[j] + " is itself + p", swap(j, b48(int.from_bytes(g[j], "big") + P))))
        if j:
            u.append((names[j] + " has bit 7 set", swap(j, bytes([g[j][0] | 0x80]) + g[j][1:])))
            u.append(("infinity with a byte in " + names[j], b"\x40" + bytes(47) + join([bytes(47) + b"\x01" if i == j else bytes(48) for i in range(1, 4)])))
        u.append((names[j] + " off by one: not on the curve", swap(j, b48(int.from_bytes(g[j], "big") + 1))))
    u.append(("bit 7 set", bytes([g[0][0] | 0x80]) + join(g)[1:]))
    u.append(("bit 5 set", bytes([g[0][0] | 0x20]) + join(g)[1:]))
    u.append(("bits 7 and 6 set on infinity", b"\xc0" + bytes(191)))
    u.append(("the sort bit with infinity", b"\x60" + bytes(191)))
    u.append(("infinity with a byte in x.c1", b"\x40" + bytes(46) + b"\x01" + bytes(144)))
    u.append(("infinity with x bits", b"\x41" + bytes(191)))
    u.append(("all zero", bytes(192)))                                # (0, 0): 0 != 4 + 4 u
    u.append(("all ones", b"\xff" * 192))
    flag = lambda b, f: bytes([b[0] | f]) + b[1:]
    c.append(("bit 7 clear", g[0] + g[1]))
    c.append(("x.c1 is p", flag(b48(P), 0x80) + g[1]))
    c.append(("x.c0 is p", flag(g[0], 0x80) + b48(P)))
    c.append(("x.c0 is itself + p", flag(g[0], 0x80) + b48(GX[0] + P)))
    c.append(("x.c0 has bit 7 set", flag(g[0], 0x80) + flag(g[1], 0x80)))
    c.append(("x.c1 is 2^381 - 1", b"\x9f" + b"\xff" * 47 + g[1]))
    c.append(("infinity with the sort bit", b"\xe0" + bytes(95)))
    c.append(("infinity with a byte in x.c1", b"\xc0" + bytes(46) + b"\x01" + bytes(48)))
    c.append(("infinity with a byte in x.c0", b"\xc0" + bytes(94) + b"\x01"))
    c.append(("x has no square root", b"\x80" + bytes(47) + b48(no_root)))
    c.append(("all zero", bytes(96)))
    c.append(("all ones", b"\xff" * 96))
    for why, b in u:
        assert decode192(b) is MALFORMED, why
    for why, b in c:
        assert decode96(b) is MALFORMED, why
    return u, c


def record(pt, **extra):
    d = dict(extra)
    d.update(uncompressed=encode192(pt).hex(), compressed=encode96(pt).hex(), in_subgroup=in_subgroup(pt))
    return d


def build_fixture():
    rng = random.Random(3812)
    ks = [0, 1, 2, 3, 4, 5, 15, 16, 17, R - 2, R - 1] + [rng.randrange(1, R) for _ in range(6)]
    u, c = malformed_records()
    off = off_subgroup_points()
    tors, cleared = h_torsion_point(), cofactor_cleared_point()
    real, imag = real_and_imaginary_y_points()
    assert real[1][1] == 0 and real[1][0] != 0 and imag[1][0] == 0 and imag[1][1] != 0 and on_curve(real) and on_curve(imag)
    assert mul(H2, tors) is INF and not in_subgroup(tors) and in_subgroup(cleared)
    fx = {
        "about": "tools/bls12_381_g2_model.py: BLS12-381 G2 in the ZCash / IETF serialisation (c1 before c0); integers are big-endian hex",
        "multiples": [record(mul(k, G), k="%x" % k) for k in ks],
        "malformed_uncompressed": [{"why": w, "bytes": b.hex()} for w, b in u],
        "malformed_compressed": [{"why": w, "bytes": b.hex()} for w, b in c],
        "off_subgroup": [record(pt) for pt in off],
        "h_torsion": record(tors),
        "cofactor_cleared": record(cleared),
        "real_y": record(real), "real_y_negated": record(neg(real)),
        "imaginary_y": record(imag), "imaginary_y_negated": record(neg(imag)),
        "field_operands": ["%096x" % v for v in field_operands()],
    }
    assert all(m["in_subgroup"] for m in fx["multiples"]) and decode96(bytes.fromhex(fx["multiples"][1]["compressed"])) == G
    for m in point_records(fx):
        pt = decode192(bytes.fromhex(m["uncompressed"]))
        assert pt is not MALFORMED and decode96(bytes.fromhex(m["compressed"])) == pt and psi_in_subgroup(pt) == m["in_subgroup"]
    return fx


def point_records(fx):
    """Every record of the fixture that is a point."""
    return fx["multiples"] + fx["off_subgroup"] + [fx[k] for k in ("h_torsion", "cofactor_cleared", "real_y", "real_y_negated", "imaginary_y", "imaginary_y_negated")]


def fixture_text():
    return json.dumps(build_fixture(), indent=1, sort_keys=True) + "\n"


if __name__ == "__main__":
    with open(FIXTURE, "w") as f:
        f.write(fixture_text())
    print(FIXTURE, file=sys.stderr)
