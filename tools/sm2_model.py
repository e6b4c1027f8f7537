#!/usr/bin/env python3
"""Host model of the SM2 signature scheme (GB/T 32918.2-2016, ISO/IEC 14888-3; RFC 8998's sm2sig_sm3) on Python integers: a pure-Python SM3 (GB/T 32905),
the curve sm2p256v1, the identity digest Z_A, signing, verification and the rule set the ecsimd_sm2_* calls promise -- written down once without any of the
library's code, so that the expected values of the GPU tests do not rest on the code under test.

    Z_A = SM3(ENTL || ID || a || b || x_G || y_G || x_A || y_A)          ENTL = the bit length of ID, two big-endian bytes
    e   = SM3(Z_A || M) as an integer (any 256-bit value where a caller hands e over)
    sign:    r = (e + x(k G)) mod n,  s = (1 + d)^-1 (k - r d) mod n
             ok = 1 <= d <= n - 2 and 1 <= k <= n - 1 and r != 0 and r + k != n and s != 0            (r = s = 0 where not)
    verify:  1 <= r, s < n;  t = (r + s) mod n != 0;  Q on the curve with x, y < p;  R = s G + t Q finite;  (e mod n + x(R) mod n) mod n == r
    pubkey:  ok = 1 <= d <= n - 2 (1 + d must be invertible), (0, 0) where not

The deterministic nonce is tools/rfc6979_model.py's (HMAC-SHA-256 over d and e, at most C(n) = 4 candidates): SM2 has no standard one, any verifier accepts
the result.  libcrypto() is OpenSSL's SM2 through ctypes, None where it does not load or does not know SM2; `--mint` writes tests/golden/sm2_vectors.json
and only where libcrypto adjudicates: every verdict in the file is libcrypto's with the model agreeing, except for public keys libcrypto cannot load
(off the curve, a coordinate >= p, (0, 0)), which are the model's and say so.  One difference, not in the mathematics: libcrypto's message-level interface
refuses an EMPTY identity, which the standard allows (ENTL = 0); such records are adjudicated at the digest level (build_fixture's lib_message).
"""
import json
import os
import random
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rfc6979_model  # noqa: E402

FIXTURE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "sm2_vectors.json")

P = 0xfffffffeffffffffffffffffffffffffffffffff00000000ffffffffffffffff
A = P - 3
B = 0x28e9fa9e9d9f5e344d5a9e4bcf6509a7f39789f515ab8f92ddbcbd414d940e93
GX = 0x32c4ae2c1f1981195f9904466a39c9948fe30bbff2660be1715a4589334c74c7
GY = 0xbc3736a2f4f6779c59bdcee36b692153d0a9877cc62a474002df32e52139f0a0
N = 0xfffffffeffffffffffffffffffffffff7203df6b21c6052b53bbf40939d54123
G = (GX, GY)
CURVE = dict(p=P, a=A, b=B, gx=GX, gy=GY, n=N)
DEFAULT_ID = b"1234567812345678"
NONCE_CAP = rfc6979_model.candidates_needed(N)          # 4
ID_LENGTHS = (0, 16, 53, 54, 61, 62, 100)               # Z_A hashes 194 + |ID| bytes: 247, 248, 255, 256 put it on 55, 56, 63, 0 modulo 64
MSG_LENGTHS = (0, 23, 24, 31, 32, 100)                  # e hashes 32 + |M| bytes: 55, 56, 63, 64
SM3_LENGTHS = (0, 1, 55, 56, 63, 64, 65, 119, 120, 128, 200)

h64 = lambda v: "%064x" % v
i2b = lambda v: v.to_bytes(32, "big")
b2i = lambda b: int.from_bytes(b, "big")


# ---- SM3
def _rotl(x, n):
    n &= 31
    return ((x << n) | (x >> (32 - n))) & 0xffffffff if n else x


def sm3(msg):
    v = [0x7380166f, 0x4914b2b9, 0x172442d7, 0xda8a0600, 0xa96f30bc, 0x163138aa, 0xe38dee4d, 0xb0fb0e4e]
    m = bytes(msg) + b"\x80" + b"\x00" * ((55 - len(msg)) % 64) + (8 * len(msg)).to_bytes(8, "big")
    for at in range(0, len(m), 64):
        w = [b2i(m[at + 4 * j:at + 4 * j + 4]) for j in range(16)]
        for j in range(16, 68):
            x = w[j - 16] ^ w[j - 9] ^ _rotl(w[j - 3], 15)
            w.append(x ^ _rotl(x, 15) ^ _rotl(x, 23) ^ _rotl(w[j - 13], 7) ^ w[j - 6])
        a, b, c, d, e, f, g, h = v
        for j in range(64):
            t = 0x79cc4519 if j < 16 else 0x7a879d8a
            a12 = _rotl(a, 12)
            ss1 = _rotl((a12 + e + _rotl(t, j)) & 0xffffffff, 7)
            ss2 = ss1 ^ a12
            ff = (a ^ b ^ c) if j < 16 else ((a & b) | (a & c) | (b & c))
            gg = (e ^ f ^ g) if j < 16 else ((e & f) | (~e & g & 0xffffffff))
            tt1 = (ff + d + ss2 + (w[j] ^ w[j + 4])) & 0xffffffff
            tt2 = (gg + h + ss1 + w[j]) & 0xffffffff
            d, c, b, a = c, _rotl(b, 9), a, tt1
            h, g, f, e = g, _rotl(f, 19), e, tt2 ^ _rotl(tt2, 9) ^ _rotl(tt2, 17)
        v = [x ^ y for x, y in zip(v, (a, b, c, d, e, f, g, h))]
    return b"".join(x.to_bytes(4, "big") for x in v)


# ---- the curve (None: the point at infinity)
def on_curve(pt):
    if pt is None:
        return False
    x, y = pt
    return 0 <= x < P and 0 <= y < P and (x, y) != (0, 0) and (y * y - (x * x * x + A * x + B)) % P == 0


def neg(pt):
    return None if pt is None else (pt[0], -pt[1] % P)


def add(p, q):
    if p is None:
        return q
    if q is None:
        return p
    if p[0] == q[0]:
        if (p[1] + q[1]) % P == 0:
            return None
        lam = (3 * p[0] * p[0] + A) * pow(2 * p[1], -1, P) % P
    else:
        lam = (q[1] - p[1]) * pow(q[0] - p[0], -1, P) % P
    x = (lam * lam - p[0] - q[0]) % P
    return x, (lam * (p[0] - x) - p[1]) % P


def _jdbl(p):
    x, y, z = p
    if z == 0 or y == 0:
        return 0, 1, 0
    yy, zz = y * y % P, z * z % P
    s = 4 * x * yy % P
    m = (3 * x * x + A * zz * zz) % P
    x3 = (m * m - 2 * s) % P
    return x3, (m * (s - x3) - 8 * yy * yy) % P, 2 * y * z % P


def _jadd_affine(p, q):
    x, y, z = p
    if z == 0:
        return q[0], q[1], 1
    zz = z * z % P
    hh, rr = (q[0] * zz - x) % P, (q[1] * zz * z - y) % P
    if hh == 0:
        return _jdbl(p) if rr == 0 else (0, 1, 0)
    h2 = hh * hh % P
    h3, v = h2 * hh % P, x * h2 % P
    x3 = (rr * rr - h3 - 2 * v) % P
    return x3, (rr * (v - x3) - y * h3) % P, z * hh % P


def mult(k, pt=G):
    """k pt for any integer k >= 0 (reduced modulo n: pt has order n or is infinity)."""
    k %= N
    if pt is None or k == 0:
        return None
    acc = (0, 1, 0)
    for bit in bin(k)[2:]:
        acc = _jdbl(acc)
        if bit == "1":
            acc = _jadd_affine(acc, pt)
    if acc[2] == 0:
        return None
    zi = pow(acc[2], -1, P)
    return acc[0] * zi * zi % P, acc[1] * zi * zi * zi % P


def lift_x(x):
    rhs = (x * x * x + A * x + B) % P
    y = pow(rhs, (P + 1) // 4, P)
    return (x, y) if y * y % P == rhs else None


# ---- the scheme
def za(q, ident=DEFAULT_ID):
    return sm3((8 * len(ident)).to_bytes(2, "big") + bytes(ident) + b"".join(i2b(v) for v in (A, B, GX, GY, q[0], q[1])))


def digest(q, ident, msg):
    return b2i(sm3(za(q, ident) + bytes(msg)))


def pubkey(d):
    if not 1 <= d <= N - 2:
        return (0, 0), 0
    return mult(d), 1


def nonce(e, d):
    kn = rfc6979_model.nonce(N, e, d, cap=NONCE_CAP) if 1 <= d < N else None
    return None if kn is None else kn[0]


def sign_digest(e, d, k=None):
    """(r, s, ok); k = None: the deterministic nonce."""
    if k is None:
        k = nonce(e, d)
    if k is None or not 1 <= d <= N - 2 or not 1 <= k <= N - 1:
        return 0, 0, 0
    r = (e + mult(k)[0]) % N
    s = pow(1 + d, -1, N) * (k - r * d) % N
    if r == 0 or r + k == N or s == 0:
        return 0, 0, 0
    return r, s, 1


def verify_digest(q, e, r, s):
    if not (1 <= r < N and 1 <= s < N) or not on_curve(q):
        return 0
    t = (r + s) % N
    if t == 0:
        return 0
    pt = add(mult(s), mult(t, q))
    if pt is None:
        return 0
    return int((e % N + pt[0] % N) % N == r)


def sign(ident, msg, d, k=None):
    q, ok = pubkey(d)
    return sign_digest(digest(q, ident, msg), d, k) if ok else (0, 0, 0)


def verify(q, ident, msg, r, s):
    return verify_digest(q, digest(q, ident, msg), r, s)


# ---- libcrypto, the adjudicator
SPKI_PREFIX = bytes.fromhex("3059301306072a8648ce3d020106082a811ccf5501822d034200")


def der_signature(r, s):
    def integer(v):
        b = v.to_bytes(max(1, (v.bit_length() + 8) // 8), "big")
        return b"\x02" + bytes([len(b)]) + b
    body = integer(r) + integer(s)
    return b"\x30" + (bytes([len(body)]) if len(body) < 128 else b"\x81" + bytes([len(body)])) + body


class _Libcrypto:
    def __init__(self, lib, C):
        self.lib, self.C = lib, C

    def _key(self, q):
        C, lib = self.C, self.lib
        if not (0 <= q[0] < 1 << 256 and 0 <= q[1] < 1 << 256):
            return None
        der = SPKI_PREFIX + b"\x04" + i2b(q[0]) + i2b(q[1])
        buf = C.create_string_buffer(der, len(der))
        pp = C.c_void_p(C.addressof(buf))
        return lib.d2i_PUBKEY(None, C.byref(pp), len(der)) or None

    def verify_digest(self, q, e, r, s):
        """1 / 0, or None where libcrypto cannot load q as a key."""
        C, lib = self.C, self.lib
        key = self._key(q)
        if key is None:
            lib.ERR_clear_error()
            return None
        ctx = lib.EVP_PKEY_CTX_new(C_void(C, key), None)
        sig, tbs = der_signature(r, s), i2b(e)
        ok = lib.EVP_PKEY_verify_init(C_void(C, ctx)) == 1 and lib.EVP_PKEY_verify(C_void(C, ctx), sig, len(sig), tbs, len(tbs)) == 1
        lib.EVP_PKEY_CTX_free(C_void(C, ctx)); lib.EVP_PKEY_free(C_void(C, key)); lib.ERR_clear_error()
        return int(ok)

    def verify(self, q, ident, msg, r, s):
        C, lib = self.C, self.lib
        key = self._key(q)
        if key is None:
            lib.ERR_clear_error()
            return None
        md, pctx = lib.EVP_MD_CTX_new(), lib.EVP_PKEY_CTX_new(C_void(C, key), None)
        sig = der_signature(r, s)
        ok = lib.EVP_PKEY_CTX_set1_id(C_void(C, pctx), bytes(ident), len(ident)) > 0
        lib.EVP_MD_CTX_set_pkey_ctx(C_void(C, md), C_void(C, pctx))
        ok = ok and lib.EVP_DigestVerifyInit(C_void(C, md), None, C_void(C, lib.EVP_sm3()), None, C_void(C, key)) == 1
        ok = ok and lib.EVP_DigestVerify(C_void(C, md), sig, len(sig), bytes(msg), len(msg)) == 1
        lib.EVP_MD_CTX_free(C_void(C, md)); lib.EVP_PKEY_CTX_free(C_void(C, pctx)); lib.EVP_PKEY_free(C_void(C, key)); lib.ERR_clear_error()
        return int(ok)


def C_void(C, v):
    return C.c_void_p(v)


def libcrypto():
    """OpenSSL's SM2 through ctypes, or None where libcrypto does not load or does not know SM2 / SM3."""
    import ctypes as C
    import ctypes.util
    name = ctypes.util.find_library("crypto")
    if not name:
        return None
    try:
        lib = C.CDLL(name)
        for fn in ("d2i_PUBKEY", "EVP_PKEY_CTX_new", "EVP_MD_CTX_new", "EVP_sm3"):
            getattr(lib, fn).restype = C.c_void_p
        for fn in ("EVP_PKEY_free", "EVP_PKEY_CTX_free", "EVP_MD_CTX_free", "EVP_MD_CTX_set_pkey_ctx", "ERR_clear_error"):
            getattr(lib, fn).restype = None
        for fn in ("EVP_PKEY_verify_init", "EVP_PKEY_verify", "EVP_PKEY_CTX_set1_id", "EVP_DigestVerifyInit", "EVP_DigestVerify"):
            getattr(lib, fn).restype = C.c_int
        lib.EVP_PKEY_verify.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t]
        lib.EVP_DigestVerify.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t]
        lib.EVP_PKEY_CTX_set1_id.argtypes = [C.c_void_p, C.c_char_p, C.c_int]
        lib.EVP_DigestVerifyInit.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.d2i_PUBKEY.argtypes = [C.c_void_p, C.c_void_p, C.c_long]
        if not lib.EVP_sm3():
            return None
        adj = _Libcrypto(lib, C)
        q = mult(EXAMPLE["d"])                                  # the standard's example must pass, else this libcrypto does not do SM2
        if adj.verify(q, DEFAULT_ID, EXAMPLE["msg"], EXAMPLE["r"], EXAMPLE["s"]) != 1 or adj.verify_digest(q, EXAMPLE["e"], EXAMPLE["r"], EXAMPLE["s"]) != 1:
            return None
        return adj
    except (OSError, AttributeError):
        return None


# ---- the standard's example (GB/T 32918.2-2016 appendix A; draft-shen-sm2-ecdsa on the recommended curve)
EXAMPLE = dict(
    d=0x3945208F7B2144B13F36E38AC6D39F95889393692860B51A42FB81EF4DF7C5B8, ident=DEFAULT_ID, msg=b"message digest",
    k=0x59276E27D506861A16680F3AD9C02DCCEF3CC1FA3CDBE4CE6D54B80DEAC1BC21,
    e=0xF0B43E94BA45ACCAACE692ED534382EB17E6AB5A19CE7B31F4486FDFC0D28640,
    r=0xF5A03B0648D2C4630EEAC513E1BB81A15944DA3827D5B74143AC7EACEEE720B3,
    s=0xB1B6AA29DF212FD8763182BC0D421CA1BB9038FD1F7F42D4840B69C485BBC1AA)
SM3_ABC = "66c7f0f462eeedd9d1f2d46bdc10e4e24167c4875cf2f7a2297da02b8f4ba8e0"
SM3_ABCD16 = "debe9ff92275b8a138604889c18e5a4d6fdb70e5387e5765293dcba39c0c5732"     # GB/T 32905 appendix A.2: "abcd" sixteen times


def high_x_point():
    """The point with x = n + 4 (< p): the least x >= n that lifts on this curve."""
    x = N
    while lift_x(x) is None:
        x += 1
    return lift_x(x)


def flip_bit(b, bit):
    b = bytearray(b)
    b[bit // 8] ^= 1 << (bit % 8)
    return bytes(b)


# ---- the fixture
def build_fixture(adj):
    """The fixture's content.  adj: libcrypto() -- every verdict is asked of it and must equal the model's (an exception says where not); None: the model alone,
    which is how the tests rebuild the file's content."""
    rng = random.Random(32918)
    rand_bytes = lambda n: bytes(rng.getrandbits(8) for _ in range(n))
    fx = dict(adjudicated_by_libcrypto=adj is not None, curve="sm2p256v1", nonce_candidates=NONCE_CAP)

    fx["sm3"] = [dict(msg=m.hex(), digest=sm3(m).hex()) for m in [b"abc", b"abcd" * 16] + [rand_bytes(n) for n in SM3_LENGTHS]]

    q = mult(EXAMPLE["d"])
    fx["example"] = dict(d=h64(EXAMPLE["d"]), id=DEFAULT_ID.hex(), msg=EXAMPLE["msg"].hex(), k=h64(EXAMPLE["k"]), qx=h64(q[0]), qy=h64(q[1]), za=za(q, DEFAULT_ID).hex(),
                         e=h64(digest(q, DEFAULT_ID, EXAMPLE["msg"])), r=h64(EXAMPLE["r"]), s=h64(EXAMPLE["s"]))

    def judged(kind, model_ok, lib_ok, note):
        if adj is not None and lib_ok is not None and lib_ok != model_ok:
            raise AssertionError(f"libcrypto says {lib_ok}, the model {model_ok}: {kind}: {note}")
        return "model" if (adj is None or lib_ok is None) and kind == "unloadable" else "libcrypto"

    # libcrypto's message-level interface does not take an EMPTY ID (EVP_PKEY_CTX_set1_id fails: its verdict is 0 whatever the signature); the standard allows
    # ENTL = 0, so those records are adjudicated at the digest level: e = SM3(Z_A || M) from the model, the verdict on (Q, e, r, s) from libcrypto.
    def lib_message(q, ident, msg, r, s):
        if adj is None:
            return None
        return adj.verify(q, ident, msg, r, s) if len(ident) else adj.verify_digest(q, digest(q, ident, msg), r, s)
    message = []
    turn = 0
    for il in ID_LENGTHS:
        for ml in MSG_LENGTHS:
            d, k, ident, msg = rng.randrange(1, N - 1), rng.randrange(1, N), rand_bytes(il), rand_bytes(ml)
            q = mult(d)
            r, s, ok = sign(ident, msg, d, k)
            assert ok == 1
            rec = dict(qx=h64(q[0]), qy=h64(q[1]), id=ident.hex(), msg=msg.hex(), r=h64(r), s=h64(s), ok=verify(q, ident, msg, r, s), note=f"valid, |ID| = {il}, |M| = {ml}")
            judged("message", rec["ok"], lib_message(q, ident, msg, r, s), rec["note"])
            message.append(rec)
            # one bit changed, the field taking turns
            fields = [f for f in ("msg", "id", "r", "s") if not (f == "msg" and ml == 0) and not (f == "id" and il == 0)]
            f = fields[turn % len(fields)]; turn += 1
            ident2, msg2, r2, s2 = ident, msg, r, s
            if f == "msg":
                msg2 = flip_bit(msg, rng.randrange(8 * ml))
            elif f == "id":
                ident2 = flip_bit(ident, rng.randrange(8 * il))
            elif f == "r":
                r2 = r ^ (1 << rng.randrange(256))
            else:
                s2 = s ^ (1 << rng.randrange(256))
            rec = dict(qx=h64(q[0]), qy=h64(q[1]), id=ident2.hex(), msg=msg2.hex(), r=h64(r2), s=h64(s2), ok=verify(q, ident2, msg2, r2, s2), note=f"one bit of {f} changed, |ID| = {il}, |M| = {ml}")
            judged("message", rec["ok"], lib_message(q, ident2, msg2, r2, s2), rec["note"])
            message.append(rec)
    fx["message"] = message

    verdicts = []

    def verdict(q, e, r, s, note, unloadable=False):
        ok = verify_digest(q, e, r, s)
        lib_ok = adj.verify_digest(q, e, r, s) if adj else None
        if adj is not None and unloadable != (lib_ok is None):
            raise AssertionError(f"libcrypto {'loads' if unloadable else 'cannot load'} the key of: {note}")
        by = judged("unloadable" if unloadable else "digest", ok, lib_ok, note)
        verdicts.append(dict(qx=h64(q[0]), qy=h64(q[1]), e=h64(e), r=h64(r), s=h64(s), ok=ok, by="model" if unloadable else by, note=note))
        return ok

    d = rng.randrange(1, N - 1)
    q = mult(d)
    e = rng.getrandbits(256)
    r, s, _ = sign_digest(e, d, rng.randrange(1, N))
    assert verdict(q, e, r, s, "valid") == 1
    for bit in (0, 255):
        assert verdict(q, e ^ (1 << bit), r, s, f"bit {bit} of e changed") == 0
    e_small = rng.getrandbits(200)
    r2, s2, _ = sign_digest(e_small, d, rng.randrange(1, N))
    assert verdict(q, e_small, r2, s2, "valid, e < 2^200") == 1
    assert verdict(q, e_small + N, r2, s2, "e >= n: the same signature under e + n, reduced modulo n") == 1
    assert verdict(q, (1 << 256) - 1, r2, s2, "e = 2^256 - 1") == 0
    big = high_x_point()
    assert big[0] == N + 4
    for y_sign in (0, 1):                                       # x(R) = n + 4: r = (e + 4) mod n; Q = t^-1 (R - s G)
        rr = big if y_sign == 0 else neg(big)
        e3 = rng.getrandbits(256)
        r3, t3 = (e3 + 4) % N, rng.randrange(1, N)
        s3 = (t3 - r3) % N
        q3 = mult(pow(t3, -1, N), add(rr, neg(mult(s3))))
        assert verdict(q3, e3, r3, s3, "x(R) = n + 4 >= n") == 1
        assert verdict(q3, e3, (r3 + 1) % N, (s3 - 1) % N, "x(R) = n + 4, r one too large (the same t)") == 0
    r4 = rng.randrange(1, N)
    assert verdict(q, e, r4, N - r4, "r + s = n: t = 0") == 0
    r5, s5 = rng.randrange(1, N), rng.randrange(1, N)
    t5 = (r5 + s5) % N
    q5 = neg(mult(s5 * pow(t5, -1, N) % N))
    assert verdict(q5, e, r5, s5, "s G + t Q is the point at infinity (Q = -(s / t) G)") == 0
    for name, rr, ss in (("r = 0", 0, s), ("r = n", N, s), ("s = 0", r, 0), ("s = n", r, N), ("r = s = 0", 0, 0), ("r + n in place of r", r + N if r + N < 1 << 256 else N, s)):
        assert verdict(q, e, rr, ss, name) == 0
    assert verdict((q[0], (q[1] + 1) % P), e, r, s, "Q off the curve (y + 1)", unloadable=True) == 0
    x0 = next(x for x in range(1 << 20) if lift_x(x) is not None)
    assert verdict((P + x0, lift_x(x0)[1]), e, r, s, f"Q's x = p + {x0}: congruent to a point of the curve, not canonical", unloadable=True) == 0
    assert verdict((q[0], q[1] + P) if q[1] + P < 1 << 256 else (q[0], P), e, r, s, "Q's y >= p", unloadable=True) == 0
    assert verdict((0, 0), e, r, s, "Q = (0, 0)", unloadable=True) == 0
    fx["digest"] = verdicts

    signs = []

    def signing(e, d, k, note):
        r, s, ok = sign_digest(e, d, k)
        q, key_ok = pubkey(d)
        if ok and adj is not None and adj.verify_digest(q, e, r, s) != 1:
            raise AssertionError(f"libcrypto refuses the model's signature: {note}")
        signs.append(dict(e=h64(e), d=h64(d), k=None if k is None else h64(k), r=h64(r), s=h64(s), ok=ok, qx=h64(q[0]), qy=h64(q[1]), key_ok=key_ok, note=note))
        return ok
    q = mult(EXAMPLE["d"])
    assert signing(EXAMPLE["e"], EXAMPLE["d"], EXAMPLE["k"], "the standard's example") == 1
    for j in range(12):
        e, d = rng.getrandbits(256), rng.randrange(1, N - 1)
        assert signing(e, d, rng.randrange(1, N) if j % 2 == 0 else None, "random, caller's nonce" if j % 2 == 0 else "random, deterministic nonce") == 1
    e = rng.getrandbits(256)
    for name, d, want in (("d = 1", 1, 1), ("d = n - 2", N - 2, 1), ("d = n - 1", N - 1, 0), ("d = 0", 0, 0), ("d = n", N, 0), ("d = 2^256 - 1", (1 << 256) - 1, 0)):
        assert signing(e, d, rng.randrange(1, N), name + ", caller's nonce") == want
        assert signing(e, d, None, name + ", deterministic nonce") == want
    d = rng.randrange(1, N - 1)
    for name, k, want in (("k = 0", 0, 0), ("k = n", N, 0), ("k = n - 1", N - 1, 1), ("k = 1", 1, 1), ("k = 2^256 - 1", (1 << 256) - 1, 0)):
        assert signing(e, d, k, name) == want
    k = rng.randrange(1, N)
    assert signing((N - k - mult(k)[0]) % N, d, k, "r + k = n") == 0
    assert signing((-mult(k)[0]) % N, d, k, "r = 0") == 0
    assert signing((1 << 256) - 1, d, k, "e = 2^256 - 1") == 1
    assert signing((1 << 256) - 1, d, None, "e = 2^256 - 1, deterministic nonce") == 1
    fx["sign"] = signs
    return fx


def dump_fixture(fx):
    return json.dumps(fx, indent=1) + "\n"


def load_fixture():
    with open(FIXTURE) as f:
        return json.load(f)


def main(argv):
    if "--mint" in argv:
        adj = libcrypto()
        if adj is None:
            print("libcrypto does not load or does not know SM2: the fixture is minted only where it adjudicates")
            return 1
        fx = build_fixture(adj)
        with open(FIXTURE, "w") as f:
            f.write(dump_fixture(fx))
        print(f"wrote {FIXTURE}: {len(fx['sm3'])} hashes, {len(fx['message'])} message records, {len(fx['digest'])} verdicts, {len(fx['sign'])} signing records")
        return 0
    q = mult(EXAMPLE["d"])
    r, s, ok = sign(DEFAULT_ID, EXAMPLE["msg"], EXAMPLE["d"], EXAMPLE["k"])
    print("example:", ok == 1 and r == EXAMPLE["r"] and s == EXAMPLE["s"] and verify(q, DEFAULT_ID, EXAMPLE["msg"], r, s) == 1, "libcrypto:", libcrypto() is not None)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
