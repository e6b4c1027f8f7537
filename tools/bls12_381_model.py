#!/usr/bin/env python3
"""bls12_381_model.py -- BLS12-381 G1 as Python integers: THE DEFINITION behind include/ecsimd_bls12_381.h.

Affine textbook group law on E: y^2 = x^3 + 4 over GF(p), the ZCash / IETF serialisation (96 bytes uncompressed, 48 compressed), the subgroup test as
[r]P = infinity, the multi-scalar multiplication as a plain sum, and a restatement of the schedule ecsimd_bls12_381_g1_msm_plan reports.  None of the
library's code.  At import the curve facts the device code relies on are asserted (primality by the Miller-Rabin below).

    python3 tools/bls12_381_model.py            writes tests/golden/bls12_381_vectors.json
"""
import json
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "bls12_381_vectors.json")

P = 0x1a0111ea397fe69a4b1ba7b6434bacd764774b84f38512bf6730d2a0f6b0f6241eabfffeb153ffffb9feffffffffaaab
R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
X = -0xd201000000010000                                              # the curve's parameter
H = 0x396c8c005555e1568c00aaab0000aaab
B = 4
GX = 0x17f1d3a73197d7942695638c4fa9ac0fc3688c4f9774b905a14e3a3f171bac586c55e83ff97a1aeffb3af00adb22c6bb
GY = 0x08b3f481e3aaa0f1a09e30ed741d8ae4fcf5e095d5d00af600db18cb2c04b3edd03cc744a2888ae40caa232946c5e7e1
G = (GX, GY)
INF = None
BETA = 0x5f19672fdf76ce51ba69c6076a0f77eaddb3a93be6f89688de17d813620a00022e01fffffffefffe
X2_2G = 0x0572cbea904d67468808c8eb50a9450c9721db309128012543902d0ac358a62ae28f75bb8f1c7c42c39a8c5529bf0f4e
MONT_R = 1 << 384                                                    # fe381.cuh's Montgomery radix
HALF = (P - 1) // 2


def is_prime(n, rounds=24):
    """Miller-Rabin with fixed bases (the first primes) and seeded random ones."""
    if n < 2:
        return False
    small = [2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37]
    for q in small:
        if n % q == 0:
            return n == q
    d, s = n - 1, 0
    while d % 2 == 0:
        d, s = d // 2, s + 1
    rng = random.Random(n & 0xffffffff)
    for a in small + [rng.randrange(2, n - 1) for _ in range(rounds)]:
        x = pow(a, d, n)
        if x in (1, n - 1):
            continue
        for _ in range(s - 1):
            x = x * x % n
            if x == n - 1:
                break
        else:
            return False
    return True


# ---- the field
def fe_sqrt(a):
    """A square root of a modulo p (p = 3 mod 4), or None."""
    a %= P
    s = pow(a, (P + 1) // 4, P)
    return s if s * s % P == a else None


def lex_largest(y):
    return y % P > HALF


# ---- the group: affine points (x, y), INF = None
def on_curve(pt):
    return pt is INF or (0 <= pt[0] < P and 0 <= pt[1] < P and (pt[1] * pt[1] - pt[0] ** 3 - B) % P == 0)


def neg(pt):
    return INF if pt is INF else (pt[0], (-pt[1]) % P)


def add(p1, p2):
    if p1 is INF:
        return p2
    if p2 is INF:
        return p1
    x1, y1 = p1
    x2, y2 = p2
    if x1 == x2:
        if (y1 + y2) % P == 0:
            return INF                                               # P + (-P), and the double of a point with y = 0
        lam = 3 * x1 * x1 * pow(2 * y1, -1, P) % P
    else:
        lam = (y2 - y1) * pow(x2 - x1, -1, P) % P
    x3 = (lam * lam - x1 - x2) % P
    return (x3, (lam * (x1 - x3) - y1) % P)


def mul(k, pt):
    """k P for an integer k >= 0: the sum is over the integers, so P need not lie in G1."""
    acc = INF
    while k:
        if k & 1:
            acc = add(acc, pt)
        pt = add(pt, pt)
        k >>= 1
    return acc


def in_subgroup(pt):
    return mul(R, pt) is INF


def endo_in_subgroup(pt):
    """phi(P) = -[x^2] P with phi(x, y) = (beta x, y): the test that halves the work; g1_check ships the definition, this is kept for comparison."""
    if pt is INF:
        return True
    return (BETA * pt[0] % P, pt[1]) == neg(mul(X * X, pt))


def msm(scalars, points, bits=256):
    acc = INF
    for k, pt in zip(scalars, points):
        acc = add(acc, mul(k % (1 << bits), pt))
    return acc


# ---- the encodings
def encode96(pt):
    if pt is INF:
        return b"\x40" + bytes(95)
    return pt[0].to_bytes(48, "big") + pt[1].to_bytes(48, "big")


def encode48(pt):
    if pt is INF:
        return b"\xc0" + bytes(47)
    b = bytearray(pt[0].to_bytes(48, "big"))
    b[0] |= 0x80 | (0x20 if lex_largest(pt[1]) else 0)
    return bytes(b)


MALFORMED = "malformed"


def decode96(b):
    """The point, INF, or MALFORMED.  On-curve only: no subgroup test."""
    assert len(b) == 96
    flags = b[0] & 0xe0
    if flags == 0x40:
        return INF if b == b"\x40" + bytes(95) else MALFORMED
    if flags != 0:
        return MALFORMED
    x, y = int.from_bytes(b[:48], "big"), int.from_bytes(b[48:], "big")
    if x >= P or y >= P or (b[48] & 0xe0) != 0:
        return MALFORMED
    return (x, y) if on_curve((x, y)) else MALFORMED


def decode48(b):
    assert len(b) == 48
    if not b[0] & 0x80:
        return MALFORMED
    if b[0] & 0x40:
        return INF if b == b"\xc0" + bytes(47) else MALFORMED
    x = int.from_bytes(bytes([b[0] & 0x1f]) + b[1:], "big")
    if x >= P:
        return MALFORMED
    y = fe_sqrt(x ** 3 + B)
    if y is None:
        return MALFORMED
    if lex_largest(y) != bool(b[0] & 0x20):
        y = (P - y) % P
    return (x, y)


# ---- the schedule (ecsimd_bls12_381_g1_msm_plan; capi.hip msm_schedule_of with 48-byte field elements and g1_lanes_schedule)
MSM_MAX_N = 1 << 24
ALG_AUTO, ALG_BUCKETS, ALG_LANES = 0, 1, 2
TREE_FAN = 16
ELEM = 48


def _ceil_log2(v):
    return 0 if v <= 1 else (v - 1).bit_length()


def _tree_passes(count):
    p = 0
    while count > 1:
        count = (count + TREE_FAN - 1) // TREE_FAN
        p += 1
    return p


def _r16(b):
    return (b + 15) // 16 * 16


def plan(n, bits, flags, threshold, elem=ELEM, planes=3):
    """The dict of ecsimd_msm_plan_t's fields, or None where the call is refused.  elem = 32 restates ecsimd_msm_plan's BUCKETS route."""
    if not (1 <= bits <= 256) or n > MSM_MAX_N or flags not in (ALG_AUTO, ALG_BUCKETS, ALG_LANES):
        return None
    route = flags if flags != ALG_AUTO else (ALG_BUCKETS if n >= threshold else ALG_LANES)
    out = dict(route=route, c=0, windows=0, buckets=0, L=0, m=0, max_chain=0, launches=1, workspace_bytes=0)
    if n == 0:
        return out
    if route == ALG_BUCKETS:
        c = min(bits, min(16, max(2, n.bit_length() - 1 - 4)))
        windows = (bits + c - 1) // c
        c = (bits + windows - 1) // windows
        L = max(4, (1 << ((_ceil_log2(n) + 1) // 2)) // 4)
        m = min(1 << c, max(2, min(32, 1 << ((c + 1) // 2))))
        T, K = n * windows, windows << c
        slices, per_window = (T + L - 1) // L, (1 << c) // m
        chunk_lanes = per_window * windows
        out.update(c=c, windows=windows, buckets=1 << c, L=L, m=m, max_chain=max(L, (n + L - 1) // L + 1, 2 * m + 2 * c, TREE_FAN, windows * (c + 1)),
                   launches=8 + _tree_passes(per_window),
                   workspace_bytes=_r16(16 + 4 * K) + _r16(4 * (K + 1)) + _r16(4 * K) + _r16(4 * T) + 32 * n + elem * n + elem * (planes - 2) * n
                   + elem * planes * (K + 2 * slices + chunk_lanes))
    else:
        assert elem == ELEM                                          # (the 256-bit LANES route is not restated here)
        out.update(max_chain=TREE_FAN, launches=3 + _tree_passes(n), workspace_bytes=16 + 3 * elem * n)
    return out


# ---- the curve facts, asserted at import
def _self_check():
    assert P.bit_length() == 381 and P % 4 == 3 and is_prime(P)
    assert R.bit_length() == 255 and is_prime(R) and R == X ** 4 - X ** 2 + 1
    assert H == (X - 1) ** 2 // 3 and (X - 1) ** 2 % 3 == 0 and H.bit_length() == 126
    assert H * R == P + 1 - (X + 1) and (H * R) % 2 == 1           # the curve's order; odd: no point has y = 0
    assert on_curve(G) and mul(R, G) is INF
    assert GY < HALF and encode48(G)[0] == 0x97 and encode48(G)[1:] == GX.to_bytes(48, "big")[1:]
    assert add(G, G)[0] == X2_2G and mul(2, G)[0] == X2_2G
    assert pow(BETA, 3, P) == 1 and BETA != 1
    assert fe_sqrt(4) == 2 or fe_sqrt(4) == P - 2
    assert (1 << 384) // P == 9                                      # a 384-bit value is below 10 p: what "any 384-bit operand" costs


_self_check()


# ---- the fixture
def curve_point(x0):
    """The first point of E with x >= x0 and the smaller y: a point of E(Fp), in G1 only by accident (probability 1 / h)."""
    x = x0
    while True:
        y = fe_sqrt(x ** 3 + B)
        if y is not None:
            return (x, min(y, P - y))
        x += 1


def off_subgroup_points(count=4):
    pts, x = [], 5
    while len(pts) < count:
        pt = curve_point(x)
        x = pt[0] + 1
        if not in_subgroup(pt):
            pts.append(pt if len(pts) % 2 == 0 else neg(pt))
    return pts


def h_torsion_point():
    """[r] Q for a point Q of E(Fp): order dividing h, not the identity, so outside G1."""
    x = 5
    while True:
        q = curve_point(x)
        t = mul(R, q)
        if t is not INF:
            assert mul(H, t) is INF and not in_subgroup(t)
            return t
        x = q[0] + 1


def field_operands():
    """The representation's bounds (fe381.cuh: every 384-bit value is accepted at the door, everything inside is canonical)."""
    top = (1 << 384) - 1
    return [0, 1, 2, P - 2, P - 1, P, P + 1, 2 * P, 9 * P, 9 * P + 1, top - 1, top, MONT_R % P, (MONT_R * MONT_R) % P, HALF, HALF + 1, 1 << 383, (1 << 381) - 1,
            int.from_bytes(b"\xff\xff\xff\xff\x00\x00\x00\x00" * 6, "big"), int.from_bytes(b"\x00\x00\x00\x00\xff\xff\xff\xff" * 6, "big")]


def malformed_records():
    gx, gy = GX.to_bytes(48, "big"), GY.to_bytes(48, "big")
    no_root = next(x for x in range(1, 100) if fe_sqrt(x ** 3 + B) is None)
    u, c = [], []
    u.append(("x is p", P.to_bytes(48, "big") + gy))
    u.append(("y is p", gx + P.to_bytes(48, "big")))
    u.append(("x is x + p", (GX + P).to_bytes(48, "big") + gy))
    u.append(("bit 7 set", bytes([gx[0] | 0x80]) + gx[1:] + gy))
    u.append(("bit 5 set", bytes([gx[0] | 0x20]) + gx[1:] + gy))
    u.append(("bits 7 and 6 set on infinity", b"\xc0" + bytes(95)))
    u.append(("infinity with a body", b"\x40" + bytes(94) + b"\x01"))
    u.append(("infinity with x bits", b"\x41" + bytes(95)))
    u.append(("flag bits in y", gx + bytes([gy[0] | 0x80]) + gy[1:]))
    u.append(("not on the curve", gx + (GY + 1).to_bytes(48, "big")))
    u.append(("all zero", bytes(96)))                                 # (0, 0): 0 != 4
    u.append(("all ones", b"\xff" * 96))
    c.append(("bit 7 clear", gx))
    c.append(("x is p", bytes([P.to_bytes(48, "big")[0] | 0x80]) + P.to_bytes(48, "big")[1:]))
    c.append(("x is 2^381 - 1", b"\x9f" + b"\xff" * 47))
    c.append(("infinity with the sign bit", b"\xe0" + bytes(47)))
    c.append(("infinity with a body", b"\xc0" + bytes(46) + b"\x01"))
    c.append(("x has no square root", bytes([0x80]) + no_root.to_bytes(48, "big")[1:]))
    c.append(("all zero", bytes(48)))
    c.append(("all ones", b"\xff" * 48))
    for why, b in u:
        assert decode96(b) is MALFORMED, why
    for why, b in c:
        assert decode48(b) is MALFORMED, why
    return u, c


def record(pt, **extra):
    d = dict(extra)
    d.update(uncompressed=encode96(pt).hex(), compressed=encode48(pt).hex(), in_subgroup=in_subgroup(pt))
    return d


def build_fixture():
    rng = random.Random(381)
    ks = [0, 1, 2, 3, 4, 5, 15, 16, 17, R - 2, R - 1] + [rng.randrange(1, R) for _ in range(8)]
    u, c = malformed_records()
    off = off_subgroup_points()
    tors = h_torsion_point()
    for pt in off + [tors]:
        assert on_curve(pt) and not in_subgroup(pt) and not endo_in_subgroup(pt)
    fx = {
        "about": "tools/bls12_381_model.py: BLS12-381 G1 in the ZCash / IETF serialisation; integers are big-endian hex",
        "multiples": [record(mul(k, G), k="%x" % k) for k in ks],
        "malformed_uncompressed": [{"why": w, "bytes": b.hex()} for w, b in u],
        "malformed_compressed": [{"why": w, "bytes": b.hex()} for w, b in c],
        "off_subgroup": [record(pt) for pt in off],
        "h_torsion": record(tors),
        "field_operands": ["%096x" % v for v in field_operands()],
    }
    assert all(m["in_subgroup"] for m in fx["multiples"]) and decode48(bytes.fromhex(fx["multiples"][1]["compressed"])) == G
    for m in fx["multiples"] + fx["off_subgroup"] + [fx["h_torsion"]]:
        pt = decode96(bytes.fromhex(m["uncompressed"]))
        assert pt is not MALFORMED and decode48(bytes.fromhex(m["compressed"])) == pt and endo_in_subgroup(pt) == m["in_subgroup"]
    return fx


def fixture_text():
    return json.dumps(build_fixture(), indent=1, sort_keys=True) + "\n"


if __name__ == "__main__":
    with open(FIXTURE, "w") as f:
        f.write(fixture_text())
    print(FIXTURE, file=sys.stderr)
