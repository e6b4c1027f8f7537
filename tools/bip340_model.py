#!/usr/bin/env python3
"""Host model of BIP-340 Schnorr signatures on secp256k1, on Python integers and `hashlib` only.

What ecsimd_hip_schnorr_sign and ecsimd_hip_schnorr_verify promise, written down once without any of the library's code, so that the expected values
of the GPU tests do not rest on the code under test: default signing (with auxiliary randomness, 32 zero bytes where the caller gives none) and
verification, for messages of any length.  Integers in and out: a key, r, s or aux is the big-endian reading of its 32 bytes.
tests/test_schnorr_cpu.py pins this model to BIP-340's test vectors 0 and 1 (tests/golden/bip340_vectors.json).

Also here: the SHA-256 midstates of the three tag blocks (the compression function in plain Python, checked against hashlib by continuing a hash from
them), which the device source holds as literals; and `chain_of_existing_calls`, verification put together from the engine's OTHER public calls, the
yardstick schnorr_verify is compared and timed against.
"""
import hashlib

P = 0xfffffffffffffffffffffffffffffffffffffffffffffffffffffffefffffc2f
N = 0xfffffffffffffffffffffffffffffffebaaedce6af48a03bbfd25e8cd0364141
GX = 0x79be667ef9dcbbac55a06295ce870b07029bfcdb2dce28d959f2815b16f81798
GY = 0x483ada7726a3c4655da4fbfc0e1108a8fd17b448a68554199c47d08ffb10d4b8
TAGS = ("BIP0340/challenge", "BIP0340/aux", "BIP0340/nonce")

# ---- SHA-256's compression function (FIPS 180-4 6.2.2), for the midstates only: everything else goes through hashlib
_K = [0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5, 0xd807aa98, 0x12835b01, 0x243185be, 0x550c7dc3,
      0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174, 0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc, 0x2de92c6f, 0x4a7484aa, 0x5cb0a9dc, 0x76f988da,
      0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147, 0x06ca6351, 0x14292967, 0x27b70a85, 0x2e1b2138, 0x4d2c6dfc, 0x53380d13,
      0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85, 0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3, 0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070,
      0x19a4c116, 0x1e376c08, 0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f, 0x682e6ff3, 0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208,
      0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2]
_IV = [0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19]
_M32 = 0xffffffff


def _rotr(x, n):
    return ((x >> n) | (x << (32 - n))) & _M32


def compress(state, block):
    """One 64-byte block into a state of eight words; returns the new state."""
    assert len(block) == 64 and len(state) == 8
    w = [int.from_bytes(block[4 * i:4 * i + 4], "big") for i in range(16)]
    for t in range(16, 64):
        s0 = _rotr(w[t - 15], 7) ^ _rotr(w[t - 15], 18) ^ (w[t - 15] >> 3)
        s1 = _rotr(w[t - 2], 17) ^ _rotr(w[t - 2], 19) ^ (w[t - 2] >> 10)
        w.append((w[t - 16] + s0 + w[t - 7] + s1) & _M32)
    a, b, c, d, e, f, g, h = state
    for t in range(64):
        t1 = (h + (_rotr(e, 6) ^ _rotr(e, 11) ^ _rotr(e, 25)) + ((e & f) ^ (~e & g & _M32)) + _K[t] + w[t]) & _M32
        t2 = ((_rotr(a, 2) ^ _rotr(a, 13) ^ _rotr(a, 22)) + ((a & b) ^ (a & c) ^ (b & c))) & _M32
        a, b, c, d, e, f, g, h = (t1 + t2) & _M32, a, b, c, (d + t1) & _M32, e, f, g
    return [(x + y) & _M32 for x, y in zip(state, (a, b, c, d, e, f, g, h))]


def midstate(tag):
    """The SHA-256 state after the 64-byte block SHA256(tag) || SHA256(tag): where every hash with that tag starts."""
    t = hashlib.sha256(tag.encode()).digest()
    return compress(_IV, t + t)


def finish_from_midstate(state, data):
    """SHA-256 of (one 64-byte block already in `state`) || data, by the plain-Python compression: what the device does with its literals."""
    total = 64 + len(data)
    padded = data + b"\x80" + b"\x00" * ((55 - len(data)) % 64) + (8 * total).to_bytes(8, "big")
    for i in range(0, len(padded), 64):
        state = compress(state, padded[i:i + 64])
    return b"".join(x.to_bytes(4, "big") for x in state)


def tagged_hash(tag, data):
    t = hashlib.sha256(tag.encode()).digest()
    return hashlib.sha256(t + t + data).digest()


# ---- the curve: Jacobian coordinates inside (no inversion per step), k G from the 256 doublings of G
def _jdbl(X, Y, Z):
    if Y == 0:
        return 0, 1, 0
    S = 4 * X * Y * Y % P
    M = 3 * X * X % P
    X3 = (M * M - 2 * S) % P
    return X3, (M * (S - X3) - 8 * pow(Y, 4, P)) % P, 2 * Y * Z % P


def _jadd_affine(X, Y, Z, x2, y2):
    if Z == 0:
        return x2, y2, 1
    Z2 = Z * Z % P
    U2, S2 = x2 * Z2 % P, y2 * Z2 * Z % P
    H, R = (U2 - X) % P, (S2 - Y) % P
    if H == 0:
        return _jdbl(X, Y, Z) if R == 0 else (0, 1, 0)
    H2 = H * H % P
    H3, V = H * H2 % P, X * H2 % P
    X3 = (R * R - H3 - 2 * V) % P
    return X3, (R * (V - X3) - Y * H3) % P, Z * H % P


def _affine(X, Y, Z):
    if Z == 0:
        return None
    zi = pow(Z, -1, P)
    return X * zi * zi % P, Y * zi * zi * zi % P


def _doublings_of_g():
    out, pt = [], (GX, GY)
    for _ in range(256):
        out.append(pt)
        pt = _affine(*_jdbl(pt[0], pt[1], 1))
    return out


_G2 = _doublings_of_g()


def mul_g(k):
    """k G as an affine point, None for k = 0 mod n."""
    k %= N
    acc = (0, 1, 0)
    for i in range(256):
        if (k >> i) & 1:
            acc = _jadd_affine(*acc, *_G2[i])
    return _affine(*acc)


def mul(k, pt):
    """k * pt (affine, or None) as an affine point."""
    k %= N
    if pt is None or k == 0:
        return None
    acc = (0, 1, 0)
    for i in range(k.bit_length() - 1, -1, -1):
        acc = _jdbl(*acc)
        if (k >> i) & 1:
            acc = _jadd_affine(*acc, *pt)
    return _affine(*acc)


def add(a, b):
    if a is None:
        return b
    if b is None:
        return a
    return _affine(*_jadd_affine(a[0], a[1], 1, b[0], b[1]))


def lift_x(x):
    """The point with that x and an even y, or None (x >= p, or no such point)."""
    if not 0 <= x < P:
        return None
    c = (pow(x, 3, P) + 7) % P
    y = pow(c, (P + 1) // 4, P)
    if y * y % P != c:
        return None
    return x, (y if y % 2 == 0 else P - y)


# ---- BIP-340
def _b(x):
    return x.to_bytes(32, "big")


def challenge(r, px, msg):
    return int.from_bytes(tagged_hash("BIP0340/challenge", _b(r) + _b(px) + msg), "big") % N


def pubkey(d):
    """x(d G), or None where d is outside [1, n - 1]."""
    return mul_g(d)[0] if 1 <= d < N else None


def sign(d, msg, aux=0, negate_nonce=True):
    """(px, r, s) of BIP-340's default signing for the secret key d, the message (bytes of any length) and the auxiliary randomness aux (an integer: its 32
    big-endian bytes; 0 = what a caller without randomness passes), or None where d is outside [1, n - 1] or the nonce comes out 0.
    negate_nonce=False leaves the nonce as drawn even where y(R) is odd: how the tests make signatures that every verifier must reject."""
    if not 1 <= d < N:
        return None
    px, py = mul_g(d)
    dd = d if py % 2 == 0 else N - d
    t = dd ^ int.from_bytes(tagged_hash("BIP0340/aux", _b(aux)), "big")
    k0 = int.from_bytes(tagged_hash("BIP0340/nonce", _b(t) + _b(px) + msg), "big") % N
    if k0 == 0:
        return None
    rx, ry = mul_g(k0)
    k = k0 if (ry % 2 == 0 or not negate_nonce) else N - k0
    return px, rx, (k + challenge(rx, px, msg) * dd) % N


def nonce_point_is_odd(d, msg, aux=0):
    """Whether y(k0 G) is odd for that signing (the lanes a test may turn into odd-R signatures)."""
    px, py = mul_g(d)
    dd = d if py % 2 == 0 else N - d
    t = dd ^ int.from_bytes(tagged_hash("BIP0340/aux", _b(aux)), "big")
    k0 = int.from_bytes(tagged_hash("BIP0340/nonce", _b(t) + _b(px) + msg), "big") % N
    return mul_g(k0)[1] % 2 == 1


def verify(px, msg, r, s):
    """BIP-340 Verify on integers below 2^256."""
    pt = lift_x(px)
    if pt is None or r >= P or s >= N:
        return False
    e = challenge(r, px, msg)
    R = add(mul_g(s), mul((N - e) % N, pt))
    return R is not None and R[1] % 2 == 0 and R[0] == r


# ---- the same verdicts from the engine's other public calls: sha256 of (tag block || r || px || m), sec1_decode of 02 || px, double_scalar_mult, and the
# range checks, n - e and the comparisons on the host (numpy on the 64-bit limbs).  `engine` is an ecsimd_amd.Engine; px, r, s are (n, 4) device tensors,
# msgs a 2-D uint8 device tensor.  Returns a numpy uint8 array.  Every intermediate goes through HBM, three of them through the host: the yardstick.
def _limbs(c):
    return [(c >> (64 * j)) & 0xffffffffffffffff for j in range(4)]


def _less_than(a, c):
    """a < c lane by lane: a = (n, 4) uint64 little-endian limbs, c an integer."""
    import numpy as np
    res = np.zeros(a.shape[0], dtype=bool)
    decided = np.zeros(a.shape[0], dtype=bool)
    for j in (3, 2, 1, 0):
        cj = np.uint64(_limbs(c)[j])
        lt, gt = a[:, j] < cj, a[:, j] > cj
        res |= ~decided & lt
        decided |= lt | gt
    return res


def _sub(a, b):
    """a - b modulo 2^256 on (n, 4) uint64 limbs."""
    import numpy as np
    out = np.empty_like(a)
    borrow = np.zeros(a.shape[0], dtype=np.uint64)
    with np.errstate(over="ignore"):
        for j in range(4):
            out[:, j] = a[:, j] - b[:, j] - borrow
            borrow = ((a[:, j] < b[:, j]) | ((a[:, j] == b[:, j]) & (borrow != 0))).astype(np.uint64)
    return out


def chain_of_existing_calls(engine, px, msgs, r, s):
    import numpy as np
    torch = engine.torch
    n = int(px.shape[0])
    if n == 0:
        return np.zeros(0, dtype=np.uint8)
    const = lambda c: np.tile(np.array([_limbs(c)], dtype=np.uint64), (n, 1))
    t = hashlib.sha256(b"BIP0340/challenge").digest()
    tag = torch.from_numpy(np.frombuffer(t + t, dtype=np.uint8).copy()).to(engine.tdev)
    rb, pb = engine.to_bytes_be(r).reshape(n, 32), engine.to_bytes_be(px).reshape(n, 32)      # big-endian bytes
    e = engine.to_numpy(engine.sha256(torch.cat([tag.expand(n, 64), rb, pb, msgs], dim=1).contiguous()))
    rec = torch.cat([torch.full((n, 1), 2, dtype=torch.uint8, device=engine.tdev), pb], dim=1).contiguous()
    qx, qy, lifted = engine.sec1_decode(1, rec, compressed=True)                               # 02 || px: the point with the even y
    r_h, s_h = engine.to_numpy(r), engine.to_numpy(s)
    usable = engine.to_numpy(lifted).astype(bool) & _less_than(r_h, P) & _less_than(s_h, N)
    e = np.where(_less_than(e, N)[:, None], e, _sub(e, const(N)))                              # e mod n
    u2 = np.where((usable & e.any(axis=1))[:, None], _sub(const(N), e), np.uint64(0))          # n - e, 0 staying 0
    u1 = np.where(usable[:, None], s_h, np.uint64(0))
    keep = torch.from_numpy(usable).to(engine.tdev).unsqueeze(1)                               # a key that did not lift: any point will do, the lane is refused below
    qx = torch.where(keep, qx, engine.to_device(const(GX))).contiguous()
    qy = torch.where(keep, qy, engine.to_device(const(GY))).contiguous()
    rx, ry, finite = engine.double_scalar_mult(1, engine.to_device(u1), engine.to_device(u2), qx, qy)
    rx, ry, finite = engine.to_numpy(rx), engine.to_numpy(ry), engine.to_numpy(finite).astype(bool)
    return (usable & finite & (rx == r_h).all(axis=1) & ((ry[:, 0] & np.uint64(1)) == 0)).astype(np.uint8)
