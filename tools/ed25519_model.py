#!/usr/bin/env python3
"""Ed25519 (RFC 8032, pure, no context, no prehash) in plain Python: the model the tests of ecsimd_ed25519_* take their expected values from.

The rule set is the one include/ecsimd_ed25519.h states:
  * pubkey / sign: section 5.1.5 / 5.1.6 bit for bit; the public key always comes from the seed.
  * verify: s < L; A decodes strictly (y < p, a root exists, not x = 0 with the sign bit set); the canonical encoding of [s]B - [k]A equals the 32 bytes
    of R as given (R is never decompressed: a non-canonical or off-curve R cannot match); k = SHA-512(R || A || M) mod L over the bytes as given.  The
    cofactorless equation.  reject_small_order: a lane whose A or R is one of the eight small-order encodings is refused as well.
Points are in extended coordinates (X, Y, Z, T) with the formulas of ed25519.cuh, so a few hundred lanes take seconds.

  python tools/ed25519_model.py --mint    writes tests/golden/ed25519_vectors.json (RFC 8032 7.1 TEST 1-3 and records minted from libcrypto)
  python tools/ed25519_model.py --table   writes ecsimd_amd/csrc/ed25519_base.inc (the comb's multiples of B and the field constants)
"""
import hashlib
import json
import os
import sys

P = 2**255 - 19
L = 2**252 + 27742317777372353535851937790883648493
D = (-121665 * pow(121666, P - 2, P)) % P
D2 = 2 * D % P
SQRT_M1 = pow(2, (P - 1) // 4, P)
BY = 4 * pow(5, P - 2, P) % P
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SMALL_ORDER = tuple(bytes.fromhex(h) for h in (
    "0100000000000000000000000000000000000000000000000000000000000000",
    "ecffffffffffffffffffffffffffffffffffffffffffffffffffffffffffff7f",
    "0000000000000000000000000000000000000000000000000000000000000000",
    "0000000000000000000000000000000000000000000000000000000000000080",
    "c7176a703d4dd84fba3c0b760d10670f2a2053fa2c39ccc64ec7fd7792ac037a",
    "c7176a703d4dd84fba3c0b760d10670f2a2053fa2c39ccc64ec7fd7792ac03fa",
    "26e8958fc2b227b045c3f489f2ef98f0d5dfac05d3c63339b13802886d53fc05",
    "26e8958fc2b227b045c3f489f2ef98f0d5dfac05d3c63339b13802886d53fc85"))


# ---- the field
def inv(x):
    return pow(x, P - 2, P)            # 0 -> 0


def sqrt_ratio(u, v):
    """(ok, x, corrected): x = sqrt(u / v) by u v^3 (u v^7)^((p - 5) / 8), times sqrt(-1) where v x^2 = -u (corrected); ok = 0 where there is no root (x is
    then what the chain left, as on the device)."""
    u %= P; v %= P
    x = u * pow(v, 3, P) * pow(u * pow(v, 7, P), (P - 5) // 8, P) % P
    vxx = v * x * x % P
    if vxx == u:
        return True, x, False
    if vxx == (-u) % P:
        return True, x * SQRT_M1 % P, True
    return False, x, False


# ---- the group: extended coordinates, a = -1
IDENTITY = (0, 1, 1, 0)


def pt_add(p, q):
    x1, y1, z1, t1 = p; x2, y2, z2, t2 = q
    a = (y1 - x1) * (y2 - x2) % P; b = (y1 + x1) * (y2 + x2) % P
    c = t1 * D2 % P * t2 % P; d = 2 * z1 * z2 % P
    e, f, g, h = b - a, d - c, d + c, b + a
    return (e * f % P, g * h % P, f * g % P, e * h % P)


def pt_dbl(p):
    x1, y1, z1, _ = p
    a = x1 * x1 % P; b = y1 * y1 % P; c = 2 * z1 * z1 % P
    h = a + b; e = h - (x1 + y1) ** 2; g = a - b; f = c + g
    return (e * f % P, g * h % P, f * g % P, e * h % P)


def pt_neg(p):
    return ((-p[0]) % P, p[1], p[2], (-p[3]) % P)


def pt_mul(k, p):
    q = IDENTITY
    for bit in bin(k)[2:] if k else "":
        q = pt_dbl(q)
        if bit == "1":
            q = pt_add(q, p)
    return q


def pt_eq(p, q):
    return (p[0] * q[2] - q[0] * p[2]) % P == 0 and (p[1] * q[2] - q[1] * p[2]) % P == 0


def encode(p):
    zi = inv(p[2]); x = p[0] * zi % P; y = p[1] * zi % P
    return (y | ((x & 1) << 255)).to_bytes(32, "little")


def decode(b):
    """The point of a 32-byte encoding, or None: y >= p, no root, or x = 0 with the sign bit set."""
    v = int.from_bytes(b, "little"); sign = v >> 255; y = v & (2**255 - 1)
    if y >= P:
        return None
    ok, x, _ = sqrt_ratio(y * y - 1, D * y * y + 1)
    if not ok or (x == 0 and sign):
        return None
    if (x & 1) != sign:
        x = P - x
    return (x, y, 1, x * y % P)


B = decode(BY.to_bytes(32, "little"))
assert B is not None and pt_eq(pt_mul(L, B), IDENTITY)


_BASE_POWERS = []


def base_point_mul(k):
    """[k mod L]B from the stored 2^i B: additions only."""
    if not _BASE_POWERS:
        q = B
        for _ in range(253):
            _BASE_POWERS.append(q)
            q = pt_dbl(q)
    k %= L
    acc, i = IDENTITY, 0
    while k:
        if k & 1:
            acc = pt_add(acc, _BASE_POWERS[i])
        k >>= 1; i += 1
    return acc


def base_mult(k):
    return encode(base_point_mul(k))


def double_mult(s, h, enc):
    """The encoding of [s]B + [h]P for the encoding of P, or None where P does not decode."""
    pt = decode(enc)
    return None if pt is None else encode(pt_add(base_point_mul(s), pt_mul(h % L, pt)))


def sc_reduce(b64):
    return int.from_bytes(b64, "little") % L


# ---- the scheme
def expand(seed):
    h = hashlib.sha512(seed).digest()
    a = int.from_bytes(h[:32], "little")
    a &= (1 << 254) - 8
    a |= 1 << 254
    return a, h[32:]


def pubkey(seed):
    return base_mult(expand(seed)[0])


def sign(seed, msg):
    """(signature, public key)"""
    a, prefix = expand(seed)
    pk = base_mult(a)
    r = sc_reduce(hashlib.sha512(prefix + msg).digest())
    rb = base_mult(r)
    k = sc_reduce(hashlib.sha512(rb + pk + msg).digest())
    return rb + ((r + k * a) % L).to_bytes(32, "little"), pk


def verify(pk, msg, sig, reject_small_order=False):
    if len(pk) != 32 or len(sig) != 64:
        return False
    rb, s = sig[:32], int.from_bytes(sig[32:], "little")
    if s >= L:
        return False
    a = decode(pk)
    if a is None:
        return False
    if reject_small_order and (pk in SMALL_ORDER or rb in SMALL_ORDER):
        return False
    k = sc_reduce(hashlib.sha512(rb + pk + msg).digest())
    return encode(pt_add(base_point_mul(s), pt_mul(k, pt_neg(a)))) == rb


# ---- libcrypto through ctypes (an implementation independent of this tree): None where it does not load
def libcrypto():
    import ctypes as C
    import ctypes.util
    name = ctypes.util.find_library("crypto")
    if not name:
        return None
    try:
        lib = C.CDLL(name)
        for f in ("EVP_PKEY_new_raw_private_key", "EVP_PKEY_new_raw_public_key", "EVP_MD_CTX_new"):
            getattr(lib, f).restype = C.c_void_p
    except (OSError, AttributeError):
        return None
    NID = 1087

    class Lib:
        @staticmethod
        def sign(seed, msg):
            key = lib.EVP_PKEY_new_raw_private_key(NID, None, seed, C.c_size_t(32))
            assert key
            pk = C.create_string_buffer(32); n = C.c_size_t(32)
            assert lib.EVP_PKEY_get_raw_public_key(C.c_void_p(key), pk, C.byref(n)) == 1
            ctx = lib.EVP_MD_CTX_new()
            assert lib.EVP_DigestSignInit(C.c_void_p(ctx), None, None, None, C.c_void_p(key)) == 1
            sig = C.create_string_buffer(64); n = C.c_size_t(64)
            assert lib.EVP_DigestSign(C.c_void_p(ctx), sig, C.byref(n), msg, C.c_size_t(len(msg))) == 1
            lib.EVP_MD_CTX_free(C.c_void_p(ctx)); lib.EVP_PKEY_free(C.c_void_p(key))
            return sig.raw, pk.raw

        @staticmethod
        def verify(pk, msg, sig):
            key = lib.EVP_PKEY_new_raw_public_key(NID, None, pk, C.c_size_t(32))
            if not key:
                return False
            ctx = lib.EVP_MD_CTX_new()
            ok = lib.EVP_DigestVerifyInit(C.c_void_p(ctx), None, None, None, C.c_void_p(key)) == 1
            ok = ok and lib.EVP_DigestVerify(C.c_void_p(ctx), sig, C.c_size_t(64), msg, C.c_size_t(len(msg))) == 1
            lib.EVP_MD_CTX_free(C.c_void_p(ctx)); lib.EVP_PKEY_free(C.c_void_p(key))
            return bool(ok)
    try:
        Lib.sign(bytes(32), b"")
    except Exception:
        return None
    return Lib


# RFC 8032 section 7.1, TEST 1-3
RFC8032 = (
    ("9d61b19deffd5a60ba844af492ec2cc44449c5697b326919703bac031cae7f60", "",
     "d75a980182b10ab7d54bfed3c964073a0ee172f3daa62325af021a68f707511a",
     "e5564300c360ac729086e2cc806e828a84877f1eb8e5d974d873e065224901555fb8821590a33bacc61e39701cf9b46bd25bf5f0595bbe24655141438e7a100b"),
    ("4ccd089b28ff96da9db6c346ec114e0f5b8a319f35aba624da8cf6ed4fb8a6fb", "72",
     "3d4017c3e843895a92b70aa74d1b7ebc9c982ccf2ec4968cc0cd55f12af4660c",
     "92a009a9f0d4cab8720e820b5f642540a2b27b5416503f8fb3762223ebdb69da085ac1e43e15996e458f3613d0f11d8c387b2eaeb4302aeeb00d291612bb0c00"),
    ("c5aa8df43f9f837bedb7442f31dcb7b166d38535076f094b85ce3a2e0b4458f7", "af82",
     "fc51cd8e6218a1a38da47ed00230f0580816ed13ba3303ac5deb911548908025",
     "6291d657deec24024827e69c3abe01a30ce548a284743a445e3680d7db5ac3ac18ff9b538d16f290ae67f760984dc6594a7c15e9716ed28dc027beceea1ec40a"),
)
MINT_LENGTHS = (0, 1, 79, 80, 81, 95, 96, 97, 128, 207, 208, 300)


def mint(path):
    ossl = libcrypto()
    assert ossl is not None, "libcrypto does not load here"
    cases = []
    for seed, msg, pk, sig in RFC8032:
        got = ossl.sign(bytes.fromhex(seed), bytes.fromhex(msg))
        assert got == (bytes.fromhex(sig), bytes.fromhex(pk)) == sign(bytes.fromhex(seed), bytes.fromhex(msg)), seed
        cases.append(dict(source="RFC 8032 7.1", seed=seed, message=msg, public_key=pk, signature=sig))
    for rep in range(3):
        for length in MINT_LENGTHS:
            seed = hashlib.sha256(b"ed25519 fixture seed %d %d" % (rep, length)).digest()
            msg = hashlib.shake_128(b"ed25519 fixture message %d %d" % (rep, length)).digest(length)
            sig, pk = ossl.sign(seed, msg)
            assert ossl.verify(pk, msg, sig)
            cases.append(dict(source="libcrypto", seed=seed.hex(), message=msg.hex(), public_key=pk.hex(), signature=sig.hex()))
    with open(path, "w") as f:
        json.dump(dict(comment="Ed25519 known answers: RFC 8032 7.1 TEST 1-3 (reproduced by libcrypto and by tools/ed25519_model.py) and records minted "
                               "from libcrypto's EVP_DigestSign (NID 1087) over the message lengths of tests/test_gpu_ed25519.py", cases=cases), f, indent=1)
        f.write("\n")
    return len(cases)


# ---- the device constants
def words(v):
    return ", ".join("0x%08xu" % ((v >> (32 * i)) & 0xffffffff) for i in range(8))


def affine(p):
    zi = inv(p[2])
    return p[0] * zi % P, p[1] * zi % P


def table_text():
    """ed25519_base.inc: row i (0..31) entry j (0..7) = (j + 1) 256^i B as (y + x, y - x, 2 d x y), 24 words each."""
    out = ["// ed25519_base.inc -- GENERATED by tools/ed25519_model.py --table; do not edit.  The constants of fe25519.cuh / ed25519.cuh and the comb's table:",
           "// row i (0 .. 31), entry j (0 .. 7) = (j + 1) 256^i B as (y + x, y - x, 2 d x y), eight little-endian 32-bit words each.",
           "#define ED25519_D_WORDS {%s}" % words(D), "#define ED25519_2D_WORDS {%s}" % words(D2), "#define ED25519_SQRTM1_WORDS {%s}" % words(SQRT_M1),
           "#define ED25519_L_WORDS {%s}" % words(L),
           "#define ED25519_BASE_TABLE \\"]
    row = B
    lines = []
    for i in range(32):
        q = row
        for j in range(8):
            x, y = affine(q)
            lines.append("  %s, %s, %s" % (words((y + x) % P), words((y - x) % P), words(D2 * x % P * y % P)))
            q = pt_add(q, row)
        for _ in range(8):
            row = pt_dbl(row)
    out.append(", \\\n".join(lines))
    return "\n".join(out) + "\n"


if __name__ == "__main__":
    if "--mint" in sys.argv:
        print(mint(os.path.join(ROOT, "tests", "golden", "ed25519_vectors.json")), "records")
    elif "--table" in sys.argv:
        with open(os.path.join(ROOT, "ecsimd_amd", "csrc", "ed25519_base.inc"), "w") as f:
            f.write(table_text())
    else:
        for seed, msg, pk, sig in RFC8032:
            assert sign(bytes.fromhex(seed), bytes.fromhex(msg)) == (bytes.fromhex(sig), bytes.fromhex(pk))
            assert verify(bytes.fromhex(pk), bytes.fromhex(msg), bytes.fromhex(sig))
        print("RFC 8032 7.1 TEST 1-3: ok")
