#!/usr/bin/env python3
"""Ed25519 (RFC 8032, pure, no context, no prehash) in plain Python: the model the tests of ecsimd_ed25519_* take their expected values from.

The rule set is the one include/ecsimd_ed25519.h states:
  * pubkey / sign: section 5.1.5 / 5.1.6 bit for bit; the public key always comes from the seed.
  * verify: s < L; A decodes strictly (y < p, a root exists, not x = 0 with the sign bit set); the canonical encoding of [s]B - [k]A equals the 32 bytes
    of R as given (R is never decompressed: a non-canonical or off-curve R cannot match); k = SHA-512(R || A || M) mod L over the bytes as given.  The
    cofactorless equation.  reject_small_order: a lane whose A or R is one of the eight small-order encodings is refused as well.
Points are in extended coordinates (X, Y, Z, T) with the formulas of ed25519.cuh, so a few hundred lanes take seconds.

  python tools/ed25519_model.py --mint    writes tests/golden/ed25519_vectors.json (RFC 8032 7.1 TEST 1-3 and records minted from libcrypto)
  python tools/ed25519_model.py --mint-verdicts   writes tests/golden/ed25519_verdicts.json (refused and accepted lanes of every kind, mixed-order keys
                                                  among them, each adjudicated by libcrypto; refuses to write where libcrypto and this model differ)
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


# ---- points outside the prime-order subgroup
def order_of(pt):
    """The order of a point of the torsion subgroup: 1, 2, 4 or 8."""
    for n in (1, 2, 4, 8):
        if pt_eq(pt_mul(n, pt), IDENTITY):
            return n
    raise ValueError("not a torsion point")


def torsion():
    """((encoding, point, order), ...) for the eight encodings of SMALL_ORDER, in that order: the identity first."""
    return tuple((e, decode(e), order_of(decode(e))) for e in SMALL_ORDER)


def mixed(point, tors):
    """point + tors: with point in the prime-order subgroup and tors a non-zero torsion point, a point of order 2 L, 4 L or 8 L."""
    return pt_add(point, tors)


def sign_mixed(a, r, t_a, t_r, msg):
    """(pk, sig, holds) for A = [a]B + t_a, R = [r]B + t_r, s = r + h a with h = SHA-512(R || A || M) mod L.  [s]B - [h]A = [r]B - [h]t_a, so the
    cofactorless equation holds iff t_r + [h]t_a is the identity: `holds`, computed from the torsion parts alone, h reduced modulo L first."""
    pk = encode(mixed(base_point_mul(a), t_a))
    rb = encode(mixed(base_point_mul(r), t_r))
    h = sc_reduce(hashlib.sha512(rb + pk + msg).digest())
    return pk, rb + ((r + h * a) % L).to_bytes(32, "little"), pt_eq(pt_add(t_r, pt_mul(h, t_a)), IDENTITY)


# ---- the verdict fixture: refused and accepted lanes of every kind, each adjudicated by libcrypto
VERDICTS_PATH = os.path.join(ROOT, "tests", "golden", "ed25519_verdicts.json")
DIVERGENT_KIND = "A non-canonical"
MIXED_KINDS = ("mixed A, honest R", "honest A, mixed R", "mixed A, mixed R")
MIXED_MINIMUM = 8          # accepted and refused lanes per class (order of t_a, order of t_r) that can accept; refused lanes per class that cannot


def refused_encodings():
    """Encodings of A that strict decoding refuses: y = p .. p + 18, x = 0 with the sign bit set, y without a point.  (Under a signature made for another
    key libcrypto refuses them all as well; p + 1 and 01 00 .. 00 80, which it reads as the identity, part from this rule set in the kind DIVERGENT_KIND.)"""
    le = lambda v: v.to_bytes(32, "little")
    out = [le(P + i) for i in range(19)] + [le(1 | (1 << 255)), le((P - 1) | (1 << 255)), le(2), le(2 | (1 << 255)), le(7), le((1 << 255) - 1), bytes([0xff]) * 32]
    assert all(decode(e) is None for e in out)
    return out


def _tag(text, *numbers):
    return (text + "".join(" %d" % n for n in numbers)).encode()


def _scalar(text, *numbers):
    return sc_reduce(hashlib.sha512(_tag(text, *numbers)).digest())


def _message(text, *numbers, length):
    return hashlib.shake_128(_tag(text, *numbers)).digest(length)


def can_accept(order_a, order_r):
    """t_r + [h]t_a = O has a solution h iff t_r lies in the group t_a generates; the torsion subgroup is cyclic of order 8, so iff order_r divides order_a."""
    return order_a % order_r == 0


def verdict_lanes():
    """[(kind, pk, msg, sig, extra)], extra = {} or what the mixed-order records carry: orders = [order of t_a, order of t_r] and holds, the predicate of
    sign_mixed.  Messages are at most 16 bytes; seeds, nonces and messages come from fixed strings."""
    le = lambda v: int(v).to_bytes(32, "little")
    flip = lambda b, bit: (int.from_bytes(b, "little") ^ (1 << bit)).to_bytes(len(b), "little")
    lanes = []
    add = lambda kind, pk, msg, sig, **extra: lanes.append((kind, pk, msg, sig, extra))
    # -- every length 0 .. 16, valid
    signed = []
    for length in range(17):
        seed = hashlib.sha256(_tag("ed25519 verdict seed", length)).digest()
        msg = _message("ed25519 verdict message", length, length=length)
        sig, pk = sign(seed, msg)
        signed.append((pk, msg, sig))
        add("valid", pk, msg, sig)
    # -- one signature per kind of damage, a few positions each
    for j, kind in enumerate(("flip pk", "flip R", "flip s", "flip message", "message shorter", "message longer", "s + k L", "s = L", "A refused",
                              "small-order A, honest R", "small-order R, honest A")):
        pk, msg, sig = signed[5 + j]
        s = int.from_bytes(sig[32:], "little")
        for t in range(4):
            bit = _scalar("ed25519 verdict bit", j, t)
            if kind == "flip pk":
                add(kind, flip(pk, bit % 256), msg, sig)
            elif kind == "flip R":
                add(kind, pk, msg, flip(sig[:32], bit % 256) + sig[32:])
            elif kind == "flip s":
                add(kind, pk, msg, sig[:32] + flip(sig[32:], bit % 252))
            elif kind == "flip message":
                add(kind, pk, flip(msg, bit % (8 * len(msg))), sig)
        if kind == "message shorter":
            add(kind, pk, msg[:-1], sig); add(kind, pk, b"", sig)
        elif kind == "message longer":
            add(kind, pk, msg + b"\x00", sig); add(kind, pk, msg + msg[:1], sig)
        elif kind == "s + k L":                               # the same residue written k L higher: every k that fits 256 bits; k = 14, 15 set the top three bits
            for k in range(1, 17):
                if s + k * L < 2**256:
                    add(kind, pk, msg, sig[:32] + le(s + k * L))
            assert (s + 14 * L) >> 253 == 7
        elif kind == "s = L":
            add(kind, pk, msg, sig[:32] + le(L))
        elif kind == "A refused":
            for e in refused_encodings():
                add(kind, e, msg, sig)
        elif kind == "small-order A, honest R":
            for e in SMALL_ORDER:
                add(kind, e, msg, sig)
        elif kind == "small-order R, honest A":
            for e in SMALL_ORDER:
                add(kind, pk, msg, e + sig[32:])
    # -- s at the edge of L, where the equation can be made to hold for any s: A = the identity, R = [s]B
    ident = SMALL_ORDER[0]
    for s in (L - 1, L, L + 1, 2 * L - 1, 15 * L + 1, 2**256 - 1, 2**255, 7 << 253):
        add("s around L under A = identity", ident, b"edge", base_mult(s) + le(s))                  # only s = L - 1 is below L
    # -- R non-canonical: y + p for y < 19.  y = 1 (the identity) under A = identity; y = 0 (order 4, either sign) under the A of order 4 with a message for
    # which -[h]A is that point, so that the canonical encoding beside it is accepted
    for i in range(19):
        add("R non-canonical", ident, b"m", le(P + i) + le(0))
    add("R canonical beside them", ident, b"m", ident + le(0))
    four = [e for e, _, n in torsion() if n == 4]
    for a in four:
        for r in four:
            j = 0
            while not verify(a, _tag("order four", j), r + le(0)):
                j += 1
            m = _tag("order four", j)
            add("R canonical beside them", a, m, r + le(0))
            add("R non-canonical", a, m, le(int.from_bytes(r, "little") + P) + le(0))
    # -- A non-canonical: libcrypto accepts, this rule set refuses
    for e in (le(P + 1), le(1 | (1 << 255))):
        add(DIVERGENT_KIND, e, b"", ident + le(0))
    # -- all 8 x 8 small-order pairs, s = 0, 8 messages
    for a in SMALL_ORDER:
        for r in SMALL_ORDER:
            for t in range(8):
                add("small order", a, bytes([t]), r + le(0))
    # -- mixed order
    tors = torsion()
    first_accepted = {}

    def search(kind, ia, ir):
        (_, t_a, order_a), (_, t_r, order_r) = tors[ia], tors[ir]
        pairs = sum(1 for _, _, x in tors for _, _, y in tors if (x, y) == (order_a, order_r))
        quota = max(2, -(-MIXED_MINIMUM // pairs)) if ia and ir else MIXED_MINIMUM       # per pair of torsion points; the classes' minimum follows
        want = {True: quota if can_accept(order_a, order_r) else 0, False: quota}
        a = expand(hashlib.sha256(_tag("ed25519 verdict mixed seed", ia, ir)).digest())[0]
        have, j = {True: 0, False: 0}, 0
        while have != want:
            r = _scalar("ed25519 verdict mixed nonce", ia, ir, j)
            msg = _message("ed25519 verdict mixed message", ia, ir, j, length=1 + j % 16)
            j += 1
            pk, sig, holds = sign_mixed(a, r, t_a, t_r, msg)
            if have[holds] == want[holds]:
                continue
            have[holds] += 1
            add(kind, pk, msg, sig, orders=[order_a, order_r], holds=int(holds))
            if holds and kind == MIXED_KINDS[0]:
                first_accepted.setdefault(ia, (pk, msg, sig))
    for ia in range(1, 8):
        search(MIXED_KINDS[0], ia, 0)
    for ir in range(1, 8):
        search(MIXED_KINDS[1], 0, ir)
    for ia in range(1, 8):
        for ir in range(1, 8):
            search(MIXED_KINDS[2], ia, ir)
    for ia in range(1, 8):                                     # an accepted mixed-order lane, damaged
        pk, msg, sig = first_accepted[ia]
        add("mixed A, flipped message", pk, flip(msg, ia % (8 * len(msg))), sig)
        add("mixed A, s + 1", pk, msg, sig[:32] + le((int.from_bytes(sig[32:], "little") + 1) % L))
    return lanes


def check_verdicts(records):
    """The conditions under which the fixture may exist; raises AssertionError.  Returns {kind: count}."""
    kinds = {}
    for rec in records:
        kinds[rec["kind"]] = kinds.get(rec["kind"], 0) + 1
        assert len(rec["message"]) <= 32, rec
        assert bool(rec.get("divergent")) == (rec["kind"] == DIVERGENT_KIND), rec
        if rec.get("divergent"):
            assert (rec["libcrypto"], rec["model"], rec["model_strict"]) == (1, 0, 0), rec
        else:
            assert rec["model"] == rec["libcrypto"], rec
        assert rec["model_strict"] <= rec["model"], rec
        if rec["kind"] in MIXED_KINDS:
            assert rec["model"] == rec["model_strict"] == rec["holds"], rec
            assert rec["public_key"] not in [e.hex() for e in SMALL_ORDER] and rec["signature"][:64] not in [e.hex() for e in SMALL_ORDER], rec
    verdicts = lambda kind: {r["model"] for r in records if r["kind"] == kind}
    assert verdicts("valid") == {1} and verdicts("R canonical beside them") == {1}
    assert verdicts("small order") == {0, 1} and verdicts("s around L under A = identity") == {0, 1}
    for kind in kinds:
        if kind not in MIXED_KINDS + ("valid", "R canonical beside them", "small order", "s around L under A = identity"):
            assert verdicts(kind) == {0}, kind
    assert kinds["small order"] == 512 and {r["model_strict"] for r in records if r["kind"] == "small order"} == {0}
    classes = {}
    for rec in records:
        if rec["kind"] in MIXED_KINDS:
            classes.setdefault((rec["kind"],) + tuple(rec["orders"]), [0, 0])[rec["model"]] += 1
    expected = {(MIXED_KINDS[0], n, 1) for n in (2, 4, 8)} | {(MIXED_KINDS[1], 1, n) for n in (2, 4, 8)} | {(MIXED_KINDS[2], m, n) for m in (2, 4, 8) for n in (2, 4, 8)}
    assert set(classes) == expected, sorted(classes)
    for (kind, order_a, order_r), (refused, accepted) in classes.items():
        assert refused >= MIXED_MINIMUM, (kind, order_a, order_r, refused)
        assert accepted >= MIXED_MINIMUM if can_accept(order_a, order_r) else accepted == 0, (kind, order_a, order_r, accepted)
    return kinds


def verdicts_text(records):
    head = dict(comment="Ed25519 verdicts: lanes of every kind tests/test_gpu_ed25519.py verifies, refused and accepted, each adjudicated by libcrypto's "
                        "EVP_DigestVerify (NID 1087) and by tools/ed25519_model.py (model: the default rule set, model_strict: with the small-order flag); "
                        "written by mint_verdicts, which refuses to write where the two differ on a record not marked divergent.  Mixed-order records: "
                        "A = [a]B + t_a, R = [r]B + t_r, s = r + h a; orders = [order of t_a, order of t_r]; holds = (t_r + [h mod L]t_a is the identity)")
    lines = ",\n".join(json.dumps(r, separators=(",", ":")) for r in records)
    return "{\"comment\":%s,\n\"records\":[\n%s\n]}\n" % (json.dumps(head["comment"]), lines)


def mint_verdicts(path):
    ossl = libcrypto()
    assert ossl is not None, "libcrypto does not load here"
    records = []
    for kind, pk, msg, sig, extra in verdict_lanes():
        rec = dict(kind=kind, public_key=pk.hex(), message=msg.hex(), signature=sig.hex(), libcrypto=int(ossl.verify(pk, msg, sig)),
                   model=int(verify(pk, msg, sig)), model_strict=int(verify(pk, msg, sig, True)))
        if kind == DIVERGENT_KIND:
            rec["divergent"] = True
        rec.update(extra)
        records.append(rec)
    kinds = check_verdicts(records)
    text = verdicts_text(records)
    golden = os.path.dirname(VERDICTS_PATH)
    largest = max(os.path.getsize(os.path.join(golden, f)) for f in os.listdir(golden) if f != os.path.basename(VERDICTS_PATH))
    assert len(text) < largest, (len(text), largest)
    with open(path, "w") as f:
        f.write(text)
    return kinds, len(text)


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
    if "--mint-verdicts" in sys.argv:
        kinds, size = mint_verdicts(VERDICTS_PATH)
        print(json.dumps(kinds, indent=1), sum(kinds.values()), "records,", size, "bytes")
    elif "--mint" in sys.argv:
        print(mint(os.path.join(ROOT, "tests", "golden", "ed25519_vectors.json")), "records")
    elif "--table" in sys.argv:
        with open(os.path.join(ROOT, "ecsimd_amd", "csrc", "ed25519_base.inc"), "w") as f:
            f.write(table_text())
    else:
        for seed, msg, pk, sig in RFC8032:
            assert sign(bytes.fromhex(seed), bytes.fromhex(msg)) == (bytes.fromhex(sig), bytes.fromhex(pk))
            assert verify(bytes.fromhex(pk), bytes.fromhex(msg), bytes.fromhex(sig))
        print("RFC 8032 7.1 TEST 1-3: ok")
