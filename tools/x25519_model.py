#!/usr/bin/env python3
"""X25519 (RFC 7748) and the Ed25519 key conversions in plain Python integers: the model the tests of ecsimd_x25519_* take their expected values from.

The rule set is the one include/ecsimd_x25519.h states:
  * x25519(k, u): the scalar is clamped, bit 255 of u is dropped, a non-canonical u stands for its residue, 255 ladder steps with a24 = 121665, the
    canonical x-coordinate, 32 zero bytes at infinity (no exception: the caller reads `ok`).
  * x25519_base(k): the same on u = 9, computed the way the device computes it -- [clamp(k) mod L]B on the Edwards curve (tools/ed25519_model.py), mapped by
    u = (1 + y) / (1 - y).
  * from_ed25519_pk: strict decoding, the eight small-order encodings refused, no prime-subgroup check (mixed_keys: keys that show it).  from_ed25519_seed: the clamped low half of SHA-512.

  python tools/x25519_model.py --mint    writes tests/golden/x25519_vectors.json (RFC 7748's values and records minted from libcrypto)
"""
import hashlib
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ed25519_model as ed   # noqa: E402

P, L = ed.P, ed.L
A24 = 121665
ROOT = ed.ROOT
NINE = (9).to_bytes(32, "little")
# the u-coordinates of small order (RFC 7748 section 6.1's check is for these): 0, 1, the two of order 8, p - 1, and the non-canonical p, p + 1
SMALL_ORDER_U = (0, 1, int.from_bytes(bytes.fromhex("e0eb7a7c3b41b8ae1656e3faf19fc46ada098deb9c32b1fd866205165f49b800"), "little"),
                 int.from_bytes(bytes.fromhex("5f9c95bca3508c24b1d0b1559c83ef5b04445cc4581c8e86d8224eddd09f1157"), "little"), P - 1, P, P + 1)


def le32(v):
    return int(v).to_bytes(32, "little")


def clamp(k):
    """decodeScalar25519 on an integer"""
    return (k & ((1 << 254) - 8)) | (1 << 254)


def ladder(k, u):
    """The x-coordinate of [k mod 2^255] u by RFC 7748's ladder: NO clamping, u any integer (its residue counts); 0 at infinity."""
    x1 = u % P
    x2, z2, x3, z3, swap = 1, 0, x1, 1, 0
    for t in range(254, -1, -1):
        kt = (k >> t) & 1
        swap ^= kt
        if swap:
            x2, x3, z2, z3 = x3, x2, z3, z2
        swap = kt
        a, b = (x2 + z2) % P, (x2 - z2) % P
        aa, bb = a * a % P, b * b % P
        e = (aa - bb) % P
        c, d = (x3 + z3) % P, (x3 - z3) % P
        da, cb = d * a % P, c * b % P
        x3 = (da + cb) ** 2 % P
        z3 = x1 * (da - cb) ** 2 % P
        x2 = aa * bb % P
        z2 = e * (aa + A24 * e) % P
    if swap:
        x2, x3, z2, z3 = x3, x2, z3, z2
    return x2 * pow(z2, P - 2, P) % P


def x25519(scalar, u):
    """32 bytes, 32 bytes -> 32 bytes (zeros at infinity)"""
    return le32(ladder(clamp(int.from_bytes(scalar, "little")), int.from_bytes(u, "little") & ((1 << 255) - 1)))


def ok_of(out):
    return int(any(out))


def ed_point_to_u(pt):
    """(Z + Y) / (Z - Y); 0 for the identity"""
    return (pt[2] + pt[1]) * ed.inv((pt[2] - pt[1]) % P) % P


def u_of_encoding(enc):
    """u = (1 + y) / (1 - y) on the y an Edwards encoding carries, whatever subgroup the point lies in: 0 for y = 1"""
    y = int.from_bytes(enc, "little") & ((1 << 255) - 1)
    return (1 + y) * ed.inv((1 - y) % P) % P


def mixed_keys(scalars):
    """[(a, index of T, [a]B, [a]B + T)] for each a and each of the seven non-zero torsion points T of ed.torsion(): Ed25519 public keys outside the prime-order
    subgroup, which from_ed25519_pk accepts (it checks no subgroup) and whose torsion part X25519's clamped scalar, a multiple of 8, removes."""
    tors = ed.torsion()
    out = []
    for a in scalars:
        pt = ed.base_point_mul(a)
        out += [(a, j, pt, ed.mixed(pt, tors[j][1])) for j in range(1, 8)]
    return out


def edwards_base(k):
    """The u of [k mod L]B: the Edwards route, for any integer k (0 where k is a multiple of L)."""
    return ed_point_to_u(ed.base_point_mul(k % L))


def x25519_base(scalar):
    return le32(edwards_base(clamp(int.from_bytes(scalar, "little"))))


def from_ed25519_pk(pk):
    """(u, ok): 32 bytes and 0 / 1"""
    pt = ed.decode(pk)
    if pt is None or pk in ed.SMALL_ORDER:
        return bytes(32), 0
    return le32(ed_point_to_u(pt)), 1


def from_ed25519_seed(seed):
    return le32(ed.expand(seed)[0])


# ---- the device's word arithmetic, on eight 32-bit words (what the tests emulate fe25519_mul_small and a ladder step with)
M32 = 0xffffffff


def words_of(v):
    return [(v >> (32 * i)) & M32 for i in range(8)]


def int_of(w):
    return sum(x << (32 * i) for i, x in enumerate(w))


def w_fold_carry(r, c):
    acc = r[0] + c * 38
    assert acc < 2**64
    o = [acc & M32]
    for i in range(1, 8):
        acc = (acc >> 32) + r[i]; o.append(acc & M32)
    again = (acc >> 32) * 38
    acc = o[0] + again; o[0] = acc & M32
    for i in range(1, 8):
        acc = (acc >> 32) + o[i]; o[i] = acc & M32
    assert acc >> 32 == 0, "the second fold carried out"
    return o


def w_mul_small(a, c):
    acc, r = 0, []
    for i in range(8):
        acc += a[i] * c
        assert acc < 2**64
        r.append(acc & M32); acc >>= 32
    assert acc * 38 + M32 < 2**64
    return w_fold_carry(r, acc)


def w_fold(t):
    """a 16-word product modulo p as a representative (fe25519_fold)"""
    acc, r = 0, []
    for i in range(8):
        acc += t[i] + t[8 + i] * 38
        r.append(acc & M32); acc >>= 32
    return w_fold_carry(r, acc)


def w_mul(a, b):
    v = int_of(a) * int_of(b)
    return w_fold([(v >> (32 * i)) & M32 for i in range(16)])


def w_add(a, b):
    v = int_of(a) + int_of(b)
    return w_fold_carry(words_of(v & (2**256 - 1)), v >> 256)


def w_sub(a, b):
    v = int_of(a) - int_of(b)
    for _ in range(2):
        borrow = v < 0
        v &= 2**256 - 1
        v -= 38 if borrow else 0
    assert v >= 0
    return words_of(v)


def w_ladder_step(x1, x2, z2, x3, z3):
    """one step of x25519_ladder behind its swap, on words"""
    A, B = w_add(x2, z2), w_sub(x2, z2)
    AA, BB = w_mul(A, A), w_mul(B, B)
    E = w_sub(AA, BB)
    C, D = w_add(x3, z3), w_sub(x3, z3)
    DA, CB = w_mul(D, A), w_mul(C, B)
    s, d = w_add(DA, CB), w_sub(DA, CB)
    return w_mul(AA, BB), w_mul(E, w_add(AA, w_mul_small(E, A24))), w_mul(s, s), w_mul(x1, w_mul(d, d))


# ---- libcrypto through ctypes (an implementation independent of this tree): None where it does not load
def libcrypto():
    import ctypes as C
    import ctypes.util
    name = ctypes.util.find_library("crypto")
    if not name:
        return None
    try:
        lib = C.CDLL(name)
        for f in ("EVP_PKEY_new_raw_private_key", "EVP_PKEY_new_raw_public_key", "EVP_PKEY_CTX_new"):
            getattr(lib, f).restype = C.c_void_p
    except (OSError, AttributeError):
        return None
    NID = 1034

    class Lib:
        @staticmethod
        def public(scalar):
            key = lib.EVP_PKEY_new_raw_private_key(NID, None, scalar, C.c_size_t(32))
            assert key
            pk = C.create_string_buffer(32); n = C.c_size_t(32)
            assert lib.EVP_PKEY_get_raw_public_key(C.c_void_p(key), pk, C.byref(n)) == 1
            lib.EVP_PKEY_free(C.c_void_p(key))
            return pk.raw

        @staticmethod
        def derive(scalar, u):
            """The shared secret, or None where EVP_PKEY_derive fails (the small-order u)."""
            key = lib.EVP_PKEY_new_raw_private_key(NID, None, scalar, C.c_size_t(32))
            peer = lib.EVP_PKEY_new_raw_public_key(NID, None, u, C.c_size_t(32))
            assert key and peer
            ctx = lib.EVP_PKEY_CTX_new(C.c_void_p(key), None)
            assert ctx
            out = C.create_string_buffer(32); n = C.c_size_t(32)
            good = lib.EVP_PKEY_derive_init(C.c_void_p(ctx)) == 1 and lib.EVP_PKEY_derive_set_peer(C.c_void_p(ctx), C.c_void_p(peer)) == 1
            good = good and lib.EVP_PKEY_derive(C.c_void_p(ctx), out, C.byref(n)) == 1
            lib.EVP_PKEY_CTX_free(C.c_void_p(ctx)); lib.EVP_PKEY_free(C.c_void_p(peer)); lib.EVP_PKEY_free(C.c_void_p(key))
            if hasattr(lib, "ERR_clear_error"):
                lib.ERR_clear_error()
            return out.raw if good else None
    try:
        Lib.public(bytes(32))
    except Exception:
        return None
    return Lib


# RFC 7748 section 5.2 (two vectors, the iteration) and section 6.1
RFC7748_VECTORS = (
    ("a546e36bf0527c9d3b16154b82465edd62144c0ac1fc5a18506a2244ba449ac4", "e6db6867583030db3594c1a424b15f7c726624ec26b3353b10a903a6d0ab1c4c",
     "c3da55379de9c6908e94ea4df28d084f32eccf03491c71f754b4075577a28552"),
    ("4b66e9d4d1b4673c5ad22691957d6af5c11b6421e0ea01d42ca4169e7918ba0d", "e5210f12786811d3f4b7959d0538ae2c31dbe7106fc03c3efc4cd549c715a493",
     "95cbde9476e8907d7aade45cb4b873f88b595a68799fa152e6f8f7647aac7957"))
RFC7748_ITERATED = {1: "422c8e7a6227d7bca1350b3e2bb7279f7897b87bb6854b783c60e80311ae3079", 1000: "684cf59ba83309552800ef566f2f4d3c1c3887c49360e3875f2eb94d99532c51"}
RFC7748_DH = dict(a="77076d0a7318a57d3c16c17251b26645df4c2f87ebc0992ab177fba51db92c2a", a_public="8520f0098930a754748b7ddcb43ef75a0dbf3a0d26381af4eba4a98eaa9b4e6a",
                  b="5dab087e624a8a4b79e17f8b83800ee66f3bb1292618b6fd1c2f8b27ff88e0eb", b_public="de9edb7d7b7dc1b4d35b61c2ece435373f8343c85b78674dadfc7e146f882b4f",
                  shared="4a5d9d5ba4ce2de1728e3bf480350f25e07e21c947d19e3376f09b3c1e161742")


def iterate(count):
    """RFC 7748 section 5.2's loop from k = u = 9: {iteration: k} for the iterations of RFC7748_ITERATED up to count"""
    k = u = NINE
    seen = {}
    for i in range(1, count + 1):
        k, u = x25519(k, u), k
        if i in RFC7748_ITERATED:
            seen[i] = k
    return seen


def on_curve(u):
    u %= P
    return pow((u * u * u + 486662 * u * u + u) % P, (P - 1) // 2, P) in (0, 1)


def edge_us():
    """the u every list of edge cases here starts from: 9, the small-order ones, the non-canonical p - 3 .. p + 18, 2^255 - 1; bit 255 clear and set"""
    us = [9] + list(SMALL_ORDER_U) + [P - 3 + i for i in range(22)] + [2**255 - 1]
    return [le32(u) for u in us] + [le32(u | (1 << 255)) for u in us]


def mint(path):
    ossl = libcrypto()
    assert ossl is not None, "libcrypto does not load here"
    cases = []
    for k, u, out in RFC7748_VECTORS:
        assert ossl.derive(bytes.fromhex(k), bytes.fromhex(u)) == bytes.fromhex(out) == x25519(bytes.fromhex(k), bytes.fromhex(u)), k
        cases.append(dict(source="RFC 7748 5.2", scalar=k, u=u, out=out, ok=1))
    d = RFC7748_DH
    for k, pub, peer in ((d["a"], d["a_public"], d["b_public"]), (d["b"], d["b_public"], d["a_public"])):
        assert ossl.public(bytes.fromhex(k)).hex() == pub == x25519_base(bytes.fromhex(k)).hex()
        assert ossl.derive(bytes.fromhex(k), bytes.fromhex(peer)).hex() == d["shared"]
        cases.append(dict(source="RFC 7748 6.1", scalar=k, u=NINE.hex(), out=pub, ok=1))
        cases.append(dict(source="RFC 7748 6.1", scalar=k, u=peer, out=d["shared"], ok=1))
    assert {i: v.hex() for i, v in iterate(1000).items()} == RFC7748_ITERATED
    twist = curve = 0
    j = 0
    while twist < 12 or curve < 12:
        k = hashlib.sha256(b"x25519 fixture scalar %d" % j).digest()
        u = hashlib.sha256(b"x25519 fixture u %d" % j).digest()
        j += 1
        if on_curve(int.from_bytes(u, "little") & (2**255 - 1)):
            if curve >= 12:
                continue
            curve += 1; kind = "curve"
        else:
            if twist >= 12:
                continue
            twist += 1; kind = "twist"
        out = ossl.derive(k, u)
        assert out == x25519(k, u)
        cases.append(dict(source="libcrypto, a point of the " + kind, scalar=k.hex(), u=u.hex(), out=out.hex(), ok=1))
    for j, u in enumerate(edge_us()):
        k = hashlib.sha256(b"x25519 fixture edge %d" % j).digest()
        out = ossl.derive(k, u)
        mine = x25519(k, u)
        assert (out is None and not any(mine)) or out == mine, u.hex()
        cases.append(dict(source="libcrypto, edge u" + ("" if out else " (EVP_PKEY_derive fails)"), scalar=k.hex(), u=u.hex(), out=mine.hex(), ok=ok_of(mine)))
    with open(path, "w") as f:
        json.dump(dict(comment="X25519 known answers: RFC 7748 5.2 and 6.1 (reproduced by libcrypto and by tools/x25519_model.py) and records minted from "
                               "libcrypto's EVP_PKEY_derive (NID 1034): points of the curve, of its twist, and the edge u of tests/test_gpu_x25519.py; ok = 0 "
                               "where libcrypto fails and this library writes zeros",
                       iterated=RFC7748_ITERATED, dh=RFC7748_DH, cases=cases), f, indent=1)
        f.write("\n")
    return len(cases)


if __name__ == "__main__":
    if "--mint" in sys.argv:
        print(mint(os.path.join(ROOT, "tests", "golden", "x25519_vectors.json")), "records")
    else:
        for k, u, out in RFC7748_VECTORS:
            assert x25519(bytes.fromhex(k), bytes.fromhex(u)).hex() == out
        assert x25519_base(bytes.fromhex(RFC7748_DH["a"])).hex() == RFC7748_DH["a_public"]
        print("RFC 7748 5.2 and 6.1: ok")
