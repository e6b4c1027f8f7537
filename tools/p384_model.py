#!/usr/bin/env python3
"""p384_model.py -- the definition of what the ecsimd_p384_* calls compute (include/ecsimd_p384.h), in Python integers.

NIST P-384 (FIPS 186-4 D.1.2.4): the affine group law, the complete projective formulas of Renes, Costello and Batina (2016, Algorithms 4 - 6 for a = -3) as
the device writes them, SHA-384 and HMAC from hashlib / hmac, RFC 6979 with ONE candidate, the verification rule set of the header, and libcrypto() -- the
adjudicator through ctypes (None where libcrypto does not load).  Integers cross as 48 big-endian bytes, a point as X || Y, a signature as r || s.

  python tools/p384_model.py --mint     writes tests/golden/p384_vectors.json (every k G, d peer and verdict from libcrypto, the model agreeing)
"""
import hashlib
import hmac
import json
import os
import random
import sys

P = 2 ** 384 - 2 ** 128 - 2 ** 96 + 2 ** 32 - 1
N = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFC7634D81F4372DDF581A0DB248B0A77AECEC196ACCC52973
B = 0xB3312FA7E23EE7E4988E056BE3F82D19181D9C6EFE8141120314088F5013875AC656398D8A2ED19D2A85C8EDD3EC2AEF
GX = 0xAA87CA22BE8B05378EB1C71EF320AD746E1D3B628BA79B9859F741E082542A385502F25DBF55296C3A545E3872760AB7
GY = 0x3617DE4A96262C6F5D9E98BF9292DC29F8F41DBD289A147CE9DA3113B5F0B8C00A60B1CE1D7E819D7A431D7C90EA0E5F
G = (GX, GY)
INF = None                                      # the identity of the affine law

FIXTURE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "p384_vectors.json")


def i2b(v):
    return int(v).to_bytes(48, "big")


def b2i(b):
    return int.from_bytes(b, "big")


# ---- the affine law
def on_curve(pt):
    if pt is INF:
        return True
    x, y = pt
    return 0 <= x < P and 0 <= y < P and (y * y - (x * x * x - 3 * x + B)) % P == 0


def neg(pt):
    return INF if pt is INF else (pt[0], (-pt[1]) % P)


def add(p, q):
    if p is INF:
        return q
    if q is INF:
        return p
    (x1, y1), (x2, y2) = p, q
    if x1 == x2:
        if (y1 + y2) % P == 0:
            return INF
        lam = (3 * x1 * x1 - 3) * pow(2 * y1, -1, P) % P
    else:
        lam = (y2 - y1) * pow(x2 - x1, -1, P) % P
    x3 = (lam * lam - x1 - x2) % P
    return (x3, (lam * (x1 - x3) - y1) % P)


# ---- the complete projective law (Renes - Costello - Batina 2016, a = -3), as p384.cuh writes it.  The identity is (0 : 1 : 0).
def _rcb_tail(t0, t1, t2, t3, t4, y3):
    # Algorithm 4 from step 19 on: t0 = X1 X2, t1 = Y1 Y2, t2 = Z1 Z2, t3 = X1 Y2 + X2 Y1, t4 = Y1 Z2 + Y2 Z1, y3 = X1 Z2 + X2 Z1
    z3 = B * t2 % P; x3 = (y3 - z3) % P; z3 = 2 * x3 % P
    x3 = (x3 + z3) % P; z3 = (t1 - x3) % P; x3 = (t1 + x3) % P
    y3 = B * y3 % P; t1 = 2 * t2 % P; t2 = (t1 + t2) % P
    y3 = (y3 - t2) % P; y3 = (y3 - t0) % P; t1 = 2 * y3 % P
    y3 = (t1 + y3) % P; t1 = 2 * t0 % P; t0 = (t1 + t0) % P
    t0 = (t0 - t2) % P; t1 = t4 * y3 % P; t2 = t0 * y3 % P
    y3 = x3 * z3 % P; y3 = (y3 + t2) % P; x3 = t3 * x3 % P
    x3 = (x3 - t1) % P; z3 = t4 * z3 % P; t1 = t3 * t0 % P
    z3 = (z3 + t1) % P
    return (x3, y3, z3)


def proj_add(p, q):
    """Algorithm 4: any two points, the identity and P = +-Q included."""
    (X1, Y1, Z1), (X2, Y2, Z2) = p, q
    t0, t1, t2 = X1 * X2 % P, Y1 * Y2 % P, Z1 * Z2 % P
    t3 = ((X1 + Y1) * (X2 + Y2) - t0 - t1) % P
    t4 = ((Y1 + Z1) * (Y2 + Z2) - t1 - t2) % P
    y3 = ((X1 + Z1) * (X2 + Z2) - t0 - t2) % P
    return _rcb_tail(t0, t1, t2, t3, t4, y3)


def proj_add_mixed(p, q):
    """Algorithm 5: q = (x2, y2) affine, not the identity; p anything."""
    (X1, Y1, Z1), (X2, Y2) = p, q
    t0, t1 = X1 * X2 % P, Y1 * Y2 % P
    t3 = ((X2 + Y2) * (X1 + Y1) - t0 - t1) % P
    t4 = (Y2 * Z1 + Y1) % P
    y3 = (X2 * Z1 + X1) % P
    return _rcb_tail(t0, t1, Z1, t3, t4, y3)


def proj_dbl(p):
    """Algorithm 6."""
    X, Y, Z = p
    t0, t1, t2 = X * X % P, Y * Y % P, Z * Z % P
    t3 = 2 * X * Y % P; z3 = 2 * X * Z % P
    y3 = (B * t2 - z3) % P; x3 = 2 * y3 % P; y3 = (x3 + y3) % P
    x3 = (t1 - y3) % P; y3 = (t1 + y3) % P; y3 = x3 * y3 % P
    x3 = x3 * t3 % P; t3 = 2 * t2 % P; t2 = (t2 + t3) % P
    z3 = (B * z3 - t2 - t0) % P; t3 = 2 * z3 % P; z3 = (z3 + t3) % P
    t3 = 2 * t0 % P; t0 = (t3 + t0 - t2) % P; t0 = t0 * z3 % P
    y3 = (y3 + t0) % P; t0 = 2 * Y * Z % P; z3 = t0 * z3 % P
    x3 = (x3 - z3) % P; z3 = 4 * t0 * t1 % P
    return (x3, y3, z3)


def to_proj(pt):
    return (0, 1, 0) if pt is INF else (pt[0], pt[1], 1)


def from_proj(p):
    X, Y, Z = p
    if Z % P == 0:
        return INF
    zi = pow(Z, -1, P)
    return (X * zi % P, Y * zi % P)


# ---- Jacobian doubling and addition (the textbook incomplete law; used only to cross-check the other two)
def jac_dbl(p):
    X, Y, Z = p
    if Z == 0 or Y == 0:
        return (1, 1, 0)
    d, g = Z * Z % P, Y * Y % P
    bb = X * g % P
    a = 3 * (X - d) * (X + d) % P
    x3 = (a * a - 8 * bb) % P
    return (x3, (a * (4 * bb - x3) - 8 * g * g) % P, ((Y + Z) ** 2 - g - d) % P)


def jac_add(p, q):
    if p[2] == 0:
        return q
    if q[2] == 0:
        return p
    (X1, Y1, Z1), (X2, Y2, Z2) = p, q
    z1z1, z2z2 = Z1 * Z1 % P, Z2 * Z2 % P
    u1, u2 = X1 * z2z2 % P, X2 * z1z1 % P
    s1, s2 = Y1 * Z2 * z2z2 % P, Y2 * Z1 * z1z1 % P
    if u1 == u2:
        return jac_dbl(p) if s1 == s2 else (1, 1, 0)
    h, r = (u2 - u1) % P, (s2 - s1) % P
    x3 = (r * r - h ** 3 - 2 * u1 * h * h) % P
    return (x3, (r * (u1 * h * h - x3) - s1 * h ** 3) % P, h * Z1 * Z2 % P)


def from_jac(p):
    if p[2] == 0:
        return INF
    zi = pow(p[2], -1, P)
    return (p[0] * zi * zi % P, p[1] * zi ** 3 % P)


def mult_affine(k, pt=G):
    """k pt by double-and-add on the affine law; k any integer, taken modulo n."""
    k %= N
    r = INF
    for bit in bin(k)[2:] if k else "":
        r = add(r, r)
        if bit == "1":
            r = add(r, pt)
    return r


def mult(k, pt=G):
    """k pt by double-and-add on the Jacobian law (one inversion; what every call below uses); k any integer, taken modulo n."""
    k %= N
    if pt is INF:
        return INF
    r = (1, 1, 0)
    for bit in bin(k)[2:] if k else "":
        r = jac_dbl(r)
        if bit == "1":
            r = jac_add(r, (pt[0], pt[1], 1))
    return from_jac(r)


def recode_signed4(k):
    """The 97 digits in [-8, 8) of 0 <= k < 2^384, least significant first, as the device's window loops take them (the last one is 0 or 1)."""
    out, carry = [], 0
    for i in range(96):
        d = ((k >> (4 * i)) & 15) + carry
        carry = 1 if d >= 8 else 0
        out.append(d - 16 * carry)
    out.append(carry)
    return out


def mult_windowed(k, pt=G):
    """k pt as the device's variable-base loop walks it: signed 4-bit windows over 1 .. 8 pt, complete additions throughout."""
    k %= N
    table = [(0, 1, 0), to_proj(pt)]
    for j in range(2, 9):
        table.append(proj_dbl(table[j // 2]) if j % 2 == 0 else proj_add(table[j - 1], table[1]))
    acc = (0, 1, 0)
    for d in reversed(recode_signed4(k)):
        for _ in range(4):
            acc = proj_dbl(acc)
        t = table[abs(d)]
        acc = proj_add(acc, (t[0], (-t[1]) % P, t[2]) if d < 0 else t)
    return from_proj(acc)


# ---- bytes
def encode_point(pt):
    return bytes(96) if pt is INF else i2b(pt[0]) + i2b(pt[1])


def decode_point(b):
    """The point of 96 bytes X || Y, or None: x, y < p and on the curve (the cofactor is 1: that is full validation)."""
    x, y = b2i(b[:48]), b2i(b[48:])
    if x >= P or y >= P or not on_curve((x, y)):
        return None
    return (x, y)


def sha384(m):
    return hashlib.sha384(m).digest()


# ---- the calls
def pubkey(d):
    """(pub, ok) of the 48-byte private key d."""
    x = b2i(d)
    if not 1 <= x < N:
        return bytes(96), 0
    return encode_point(mult(x)), 1


def ecdh(d, peer):
    """(z, ok): z = x(d peer)."""
    x, q = b2i(d), decode_point(peer)
    if not 1 <= x < N or q is None:
        return bytes(48), 0
    return i2b(mult(x, q)[0]), 1


def rfc6979_k(x, digest):
    """The FIRST candidate of RFC 6979 section 3.2 with HMAC-SHA-384 (hlen = qlen = 384), or None where it is 0 or >= n (probability below 2^-194)."""
    h1 = i2b(b2i(digest) % N)                     # bits2octets: one conditional subtraction of n
    V, K = b"\x01" * 48, b"\x00" * 48
    K = hmac.new(K, V + b"\x00" + i2b(x) + h1, hashlib.sha384).digest()
    V = hmac.new(K, V, hashlib.sha384).digest()
    K = hmac.new(K, V + b"\x01" + i2b(x) + h1, hashlib.sha384).digest()
    V = hmac.new(K, V, hashlib.sha384).digest()
    V = hmac.new(K, V, hashlib.sha384).digest()
    k = b2i(V)
    return k if 1 <= k < N else None


def sign(d, digest):
    """(sig, ok): deterministic ECDSA over the 48-byte string bits2int sees."""
    x = b2i(d)
    if not 1 <= x < N:
        return bytes(96), 0
    k = rfc6979_k(x, digest)
    if k is None:
        return bytes(96), 0
    r = mult(k)[0] % N
    s = pow(k, -1, N) * (b2i(digest) + r * x) % N
    if r == 0 or s == 0:
        return bytes(96), 0
    return i2b(r) + i2b(s), 1


def verify(pub, digest, sig):
    """1 iff 1 <= r, s < n, pub decodes, u1 G + u2 Q is not the identity and x(R) mod n = r."""
    r, s = b2i(sig[:48]), b2i(sig[48:])
    q = decode_point(pub)
    if not (1 <= r < N and 1 <= s < N) or q is None:
        return 0
    w = pow(s, -1, N)
    R = add(mult(b2i(digest) * w), mult(r * w, q))
    return int(R is not INF and R[0] % N == r)


# ---- the adjudicator
def libcrypto():
    import ctypes as C
    import ctypes.util
    name = ctypes.util.find_library("crypto")
    if not name:
        return None
    try:
        lib = C.CDLL(name)
        for f in ("EC_GROUP_new_by_curve_name", "EC_POINT_new", "BN_bin2bn", "BN_new", "BN_CTX_new", "ECDSA_SIG_new", "EC_KEY_new"):
            getattr(lib, f).restype = C.c_void_p
        grp = lib.EC_GROUP_new_by_curve_name(715)
        if not grp:
            return None
    except (OSError, AttributeError):
        return None
    V = C.c_void_p

    def bn(v):
        b = i2b(v) if v < 2 ** 384 else int(v).to_bytes(96, "big")
        return lib.BN_bin2bn(b, len(b), None)

    def point_of(pt, ctx):
        p = lib.EC_POINT_new(V(grp))
        x, y = bn(pt[0]), bn(pt[1])
        ok = lib.EC_POINT_set_affine_coordinates(V(grp), V(p), V(x), V(y), V(ctx)) == 1
        lib.BN_free(V(x)); lib.BN_free(V(y))
        if not ok:
            lib.EC_POINT_free(V(p))
            return None
        return p

    def affine_of(p, ctx):
        if lib.EC_POINT_is_at_infinity(V(grp), V(p)) == 1:
            return INF
        x, y = lib.BN_new(), lib.BN_new()
        assert lib.EC_POINT_get_affine_coordinates(V(grp), V(p), V(x), V(y), V(ctx)) == 1
        out = []
        for v in (x, y):
            buf = C.create_string_buffer(48)
            assert lib.BN_bn2binpad(V(v), buf, 48) == 48
            out.append(b2i(buf.raw)); lib.BN_free(V(v))
        return tuple(out)

    class Lib:
        @staticmethod
        def mult(k, pt=None):
            """k G (pt None) or k pt by EC_POINT_mul; k < 2^768."""
            ctx = lib.BN_CTX_new(); kb = bn(k); r = lib.EC_POINT_new(V(grp))
            if pt is None:
                assert lib.EC_POINT_mul(V(grp), V(r), V(kb), None, None, V(ctx)) == 1
            else:
                q = point_of(pt, ctx); assert q
                assert lib.EC_POINT_mul(V(grp), V(r), None, V(q), V(kb), V(ctx)) == 1
                lib.EC_POINT_free(V(q))
            out = affine_of(r, ctx)
            lib.EC_POINT_free(V(r)); lib.BN_free(V(kb)); lib.BN_CTX_free(V(ctx))
            return out

        @staticmethod
        def verify(pub, digest, sig):
            """ECDSA_do_verify on the 96-byte key, the 48-byte digest and r || s; 0 where the key is refused."""
            ctx = lib.BN_CTX_new()
            q = point_of((b2i(pub[:48]), b2i(pub[48:])), ctx)
            if not q:
                lib.BN_CTX_free(V(ctx))
                return 0
            key = lib.EC_KEY_new()
            assert lib.EC_KEY_set_group(V(key), V(grp)) == 1
            ok = lib.EC_KEY_set_public_key(V(key), V(q)) == 1
            sg = lib.ECDSA_SIG_new()
            assert lib.ECDSA_SIG_set0(V(sg), V(bn(b2i(sig[:48]))), V(bn(b2i(sig[48:])))) == 1
            res = lib.ECDSA_do_verify(digest, 48, V(sg), V(key)) if ok else 0
            lib.ECDSA_SIG_free(V(sg)); lib.EC_KEY_free(V(key)); lib.EC_POINT_free(V(q)); lib.BN_CTX_free(V(ctx))
            return int(res == 1)
    try:
        if Lib.mult(1) != G:
            return None
    except Exception:
        return None
    return Lib


# ---- the fixture
RFC6979_X = 0x6B9D3DAD2E1B8C1C05B19875B6659F4DE23C3B667BF297BA9AA47740787137D896D5724E4C70A825F872C9EA60D2EDF5
EDGE_SCALARS = [1, 2, 3, 15, 16, N - 2, N - 1, 2 ** 383, 0x8888 << 300, (1 << 384) // 15 % N]


def lift_x(x):
    """A point with this x, or None."""
    y2 = (x * x * x - 3 * x + B) % P
    y = pow(y2, (P + 1) // 4, P)
    return (x, y) if y * y % P == y2 else None


def high_x_case(r):
    """(pub, digest, sig) whose R = u1 G + u2 Q has x = n + 2 >= n: valid with r = 2 (x mod n), refused with any other r."""
    R = lift_x(N + 2); assert R is not None
    s, e = 0x1234567 + 2 ** 200, b2i(sha384(b"x(R) >= n"))
    q = mult(pow(r, -1, N), add(mult(s, R), neg(mult(e))))
    return encode_point(q), i2b(e), i2b(r) + i2b(s)


def build_fixture(adj):
    """The fixture as a dict; adj = libcrypto() decides every product and verdict where it is given, and the model must agree."""
    rng = random.Random(384)
    rnd = lambda: rng.randrange(1, N)
    base, dh, signs, verdicts = [], [], [], []

    def product(k, pt=None):
        m = mult(k, G if pt is None else pt)
        if adj is not None:
            ref = adj.mult(k, pt)
            assert ref == m, ("model and libcrypto disagree on a product", hex(k))
        return m

    for k in EDGE_SCALARS + [rnd() for _ in range(30)]:
        base.append({"k": i2b(k).hex(), "pub": encode_point(product(k)).hex()})
    for j in range(40):
        d = EDGE_SCALARS[j] if j < len(EDGE_SCALARS) else rnd()
        peer = product(rnd()) if j % 8 else (G if j == 0 else neg(G))
        dh.append({"d": i2b(d).hex(), "peer": encode_point(peer).hex(), "z": i2b(product(d, peer)[0]).hex()})

    def verdict(pub, digest, sig, note, ref=None):
        ok = verify(pub, digest, sig)
        if adj is not None:
            assert adj.verify(pub, digest, sig) == ok, ("model and libcrypto disagree on a verdict", note)
        verdicts.append(dict(ref, ok=ok, note=note) if ref else {"pub": pub.hex(), "digest": digest.hex(), "sig": sig.hex(), "ok": ok, "note": note})
        return ok

    for j in range(24):
        d = RFC6979_X if j < 2 else rnd()
        msg = (b"sample", b"test")[j] if j < 2 else bytes(rng.randrange(256) for _ in range(rng.randrange(0, 48)))
        digest = sha384(msg)
        sig, ok = sign(i2b(d), digest); assert ok
        pub = pubkey(i2b(d))[0]
        signs.append({"d": i2b(d).hex(), "msg": msg.hex(), "pub": pub.hex(), "sig": sig.hex()})
        assert verdict(pub, digest, sig, "valid", {"sign": j}) == 1
        if j < 16:                                                   # one bit of each part changed: stored as (record, part, bit), see expand_fixture
            for part, bit, note in (("pub", rng.randrange(768), "pub bit"), ("digest", rng.randrange(384), "digest bit"), ("sig", rng.randrange(384), "r bit"),
                                    ("sig", 384 + rng.randrange(384), "s bit")):
                bent = dict(pub=pub, digest=digest, sig=sig); bent[part] = flip_bit(bent[part], bit)
                assert verdict(bent["pub"], bent["digest"], bent["sig"], note, {"sign": j, "part": part, "bit": bit}) == 0
    d = rnd(); pub = pubkey(i2b(d))[0]; digest = sha384(b"edges"); sig = sign(i2b(d), digest)[0]
    for note, bad in (("r = 0", bytes(48) + sig[48:]), ("s = 0", sig[:48] + bytes(48)), ("r = n", i2b(N) + sig[48:]), ("s = n", sig[:48] + i2b(N)),
                      ("r = 2^384 - 1", b"\xff" * 48 + sig[48:])):
        assert verdict(pub, digest, bad, note) == 0
    for note, dg in (("digest all ff (e >= n)", b"\xff" * 48), ("digest = n (u1 = 0)", i2b(N))):
        assert verdict(pub, dg, sign(i2b(d), dg)[0], note) == 1
    r0 = rnd()                                                       # e = -r d: u1 G + u2 Q = w (e + r d) G is the identity
    assert verdict(pub, i2b((-r0 * d) % N), i2b(r0) + i2b(rnd()), "e = -r d (the sum is the identity)") == 0
    assert verdict(*high_x_case(2), "x(R) = n + 2, r = 2") == 1
    hp, hd, hs = high_x_case(2)
    assert verdict(hp, hd, i2b(3) + hs[48:], "x(R) = n + 2, r = 3") == 0
    off = next(pt for pt in map(lift_x, range(1, 100)) if pt is not None)      # a point with x + p < 2^384: the encoding x + p is refused, x < p is the rule
    for note, bp in (("x = p", i2b(P) + pub[48:]), ("y = p", pub[:48] + i2b(P)), ("off the curve by one in y", pub[:48] + i2b((b2i(pub[48:]) + 1) % P)),
                     ("(0, 0)", bytes(96)), ("x + p", i2b(off[0] + P) + i2b(off[1]))):
        assert verdict(bp, digest, sig, "public key: " + note) == 0
    return {"curve": "P-384", "adjudicated_by_libcrypto": adj is not None, "base": base, "ecdh": dh, "sign": signs, "verify": verdicts}


def flip_bit(b, bit):
    return bytes(v ^ (1 << (bit % 8)) if q == bit // 8 else v for q, v in enumerate(b))


def expand_fixture(fx):
    """The fixture as the tests read it: every signing record with its digest (SHA-384 of its message), every verdict with pub, digest and sig in full --
    on disk a verdict about a signing record names the record and, where one bit of it was changed, the part and the bit."""
    signs = [dict(r, digest=sha384(bytes.fromhex(r["msg"])).hex()) for r in fx["sign"]]
    verdicts = []
    for v in fx["verify"]:
        if "sign" in v:
            parts = {k: bytes.fromhex(signs[v["sign"]][k]) for k in ("pub", "digest", "sig")}
            if "part" in v:
                parts[v["part"]] = flip_bit(parts[v["part"]], v["bit"])
            v = {"pub": parts["pub"].hex(), "digest": parts["digest"].hex(), "sig": parts["sig"].hex(), "ok": v["ok"], "note": v["note"]}
        verdicts.append(v)
    return dict(fx, sign=signs, verify=verdicts)


def load_fixture():
    with open(FIXTURE) as f:
        return expand_fixture(json.load(f))


def dump_fixture(fx):
    """One record per line."""
    rec = lambda r: json.dumps(r, sort_keys=True, separators=(",", ":"))
    body = ",\n".join('"%s":[\n%s\n]' % (k, ",\n".join(rec(r) for r in fx[k])) for k in ("base", "ecdh", "sign", "verify"))
    return '{"adjudicated_by_libcrypto":%s,"curve":"P-384",\n%s}\n' % (json.dumps(fx["adjudicated_by_libcrypto"]), body)


def main(argv):
    if "--mint" in argv:
        adj = libcrypto()
        if adj is None:
            sys.exit("libcrypto does not load here: the fixture is minted only where it adjudicates")
        fx = build_fixture(adj)
        with open(FIXTURE, "w") as f:
            f.write(dump_fixture(fx))
        print(f"wrote {FIXTURE}: {len(fx['base'])} products, {len(fx['ecdh'])} agreements, {len(fx['sign'])} signatures, {len(fx['verify'])} verdicts")
        return
    assert mult(N) is INF and (-pow(P, -1, 2 ** 32)) % 2 ** 32 == 1
    print("n G is the identity; -1/p mod 2^32 = 1")


if __name__ == "__main__":
    main(sys.argv[1:])
