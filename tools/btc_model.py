#!/usr/bin/env python3
"""Host model of what Bitcoin makes of SHA-256 and secp256k1: RIPEMD-160 in plain Python (a stock `hashlib` need not offer it), HASH160 and the double
SHA-256 through `hashlib.sha256`, SEC1 public-key hashes, and BIP-341's three key tweaks on Python integers.

What ecsimd_hip_ripemd160, _hash160, _sha256d, _btc_pubkey_hash, _xonly_tweak_add, _taproot_tweak_pubkey and _taproot_tweak_seckey promise, written down
once without any of the library's code.  The curve arithmetic and the tag midstate come from tools/bip340_model.py.  tests/test_btc_cpu.py pins this model
to published known answers (tests/golden/btc_vectors.json): Dobbertin, Bosselaers and Preneel's RIPEMD-160 vectors, the P2PKH hash of secret key 1, and
BIP-341's wallet vector without a script tree.

Integers in and out: a key, a tweak or a merkle root is the big-endian reading of its 32 bytes.  A refused input gives None.
"""
import hashlib

from bip340_model import GX, GY, N, P, add, lift_x, midstate, mul_g, tagged_hash   # noqa: F401  (midstate: the literal the device source holds)

TAG = "TapTweak"

# ---- RIPEMD-160 (Dobbertin, Bosselaers, Preneel 1996): two lines of five rounds of sixteen steps over one little-endian block
_RL = [list(range(16)),
       [7, 4, 13, 1, 10, 6, 15, 3, 12, 0, 9, 5, 2, 14, 11, 8],
       [3, 10, 14, 4, 9, 15, 8, 1, 2, 7, 0, 6, 13, 11, 5, 12],
       [1, 9, 11, 10, 0, 8, 12, 4, 13, 3, 7, 15, 14, 5, 6, 2],
       [4, 0, 5, 9, 7, 12, 2, 10, 14, 1, 3, 8, 11, 6, 15, 13]]
_RR = [[5, 14, 7, 0, 9, 2, 11, 4, 13, 6, 15, 8, 1, 10, 3, 12],
       [6, 11, 3, 7, 0, 13, 5, 10, 14, 15, 8, 12, 4, 9, 1, 2],
       [15, 5, 1, 3, 7, 14, 6, 9, 11, 8, 12, 2, 10, 0, 4, 13],
       [8, 6, 4, 1, 3, 11, 15, 0, 5, 12, 2, 13, 9, 7, 10, 14],
       [12, 15, 10, 4, 1, 5, 8, 7, 6, 2, 13, 14, 0, 3, 9, 11]]
_SL = [[11, 14, 15, 12, 5, 8, 7, 9, 11, 13, 14, 15, 6, 7, 9, 8],
       [7, 6, 8, 13, 11, 9, 7, 15, 7, 12, 15, 9, 11, 7, 13, 12],
       [11, 13, 6, 7, 14, 9, 13, 15, 14, 8, 13, 6, 5, 12, 7, 5],
       [11, 12, 14, 15, 14, 15, 9, 8, 9, 14, 5, 6, 8, 6, 5, 12],
       [9, 15, 5, 11, 6, 8, 13, 12, 5, 12, 13, 14, 11, 8, 5, 6]]
_SR = [[8, 9, 9, 11, 13, 15, 15, 5, 7, 7, 8, 11, 14, 14, 12, 6],
       [9, 13, 15, 7, 12, 8, 9, 11, 7, 7, 12, 7, 6, 15, 13, 11],
       [9, 7, 15, 11, 8, 6, 6, 14, 12, 13, 5, 14, 13, 13, 7, 5],
       [15, 5, 8, 11, 14, 14, 6, 14, 6, 9, 12, 9, 12, 5, 15, 8],
       [8, 5, 12, 9, 12, 5, 14, 6, 8, 13, 6, 5, 15, 13, 11, 11]]
_KL = [0x00000000, 0x5a827999, 0x6ed9eba1, 0x8f1bbcdc, 0xa953fd4e]
_KR = [0x50a28be6, 0x5c4dd124, 0x6d703ef3, 0x7a6d76e9, 0x00000000]
RMD_IV = [0x67452301, 0xefcdab89, 0x98badcfe, 0x10325476, 0xc3d2e1f0]
_M32 = 0xffffffff


def _rol(x, n):
    return ((x << n) | (x >> (32 - n))) & _M32


def _f(j, x, y, z):
    if j == 0:
        return x ^ y ^ z
    if j == 1:
        return (x & y) | (~x & z & _M32)
    if j == 2:
        return (x | (~y & _M32)) ^ z
    if j == 3:
        return (x & z) | (y & ~z & _M32)
    return x ^ (y | (~z & _M32))


def rmd_compress(state, block):
    """One 64-byte block into a state of five words; returns the new state."""
    assert len(block) == 64 and len(state) == 5
    w = [int.from_bytes(block[4 * i:4 * i + 4], "little") for i in range(16)]
    al, bl, cl, dl, el = state
    ar, br, cr, dr, er = state
    for rnd in range(5):
        for i in range(16):
            t = (_rol((al + _f(rnd, bl, cl, dl) + w[_RL[rnd][i]] + _KL[rnd]) & _M32, _SL[rnd][i]) + el) & _M32
            al, el, dl, cl, bl = el, dl, _rol(cl, 10), bl, t
            t = (_rol((ar + _f(4 - rnd, br, cr, dr) + w[_RR[rnd][i]] + _KR[rnd]) & _M32, _SR[rnd][i]) + er) & _M32
            ar, er, dr, cr, br = er, dr, _rol(cr, 10), br, t
    h0, h1, h2, h3, h4 = state
    return [(h1 + cl + dr) & _M32, (h2 + dl + er) & _M32, (h3 + el + ar) & _M32, (h4 + al + br) & _M32, (h0 + bl + cr) & _M32]


def ripemd160(msg):
    padded = msg + b"\x80" + b"\x00" * ((55 - len(msg)) % 64) + (8 * len(msg)).to_bytes(8, "little")
    state = RMD_IV
    for i in range(0, len(padded), 64):
        state = rmd_compress(state, padded[i:i + 64])
    return b"".join(x.to_bytes(4, "little") for x in state)


def sha256d(msg):
    return hashlib.sha256(hashlib.sha256(msg).digest()).digest()


def hash160(msg):
    return ripemd160(hashlib.sha256(msg).digest())


def sec1(x, y, compressed=True):
    """The SEC1 encoding of the integers as they are: no validation, as in the device call."""
    return (bytes([2 | (y & 1)]) + x.to_bytes(32, "big")) if compressed else (b"\x04" + x.to_bytes(32, "big") + y.to_bytes(32, "big"))


def btc_pubkey_hash(x, y, compressed=True):
    return hash160(sec1(x, y, compressed))


# ---- BIP-341
def _b(x):
    return x.to_bytes(32, "big")


def tap_tweak(px, merkle_root=None):
    """int(H_TapTweak(px || merkle_root)), NOT reduced modulo n; merkle_root None: the key-path-only form, 32 bytes of data."""
    return int.from_bytes(tagged_hash(TAG, _b(px) + (b"" if merkle_root is None else _b(merkle_root))), "big")


def xonly_tweak_add(px, t):
    """(x(Q), parity of y(Q)) for Q = lift_x(px) + t G, or None where px does not lift, t >= n or Q is infinite.  t = 0 gives Q = lift_x(px)."""
    pt = lift_x(px) if 0 <= px < 2**256 else None
    if pt is None or not 0 <= t < N:
        return None
    q = add(pt, mul_g(t))
    return None if q is None else (q[0], q[1] & 1)


def taproot_tweak_pubkey(px, merkle_root=None):
    if not 0 <= px < P:
        return None
    return xonly_tweak_add(px, tap_tweak(px, merkle_root))


def taproot_tweak_seckey(d, merkle_root=None):
    """(d_out, px): the secret key of the output key and the internal x-only key, or None where d is outside [1, n - 1], the tweak is >= n or the sum is 0."""
    if not 1 <= d < N:
        return None
    px, py = mul_g(d)
    dd = d if py % 2 == 0 else N - d
    t = tap_tweak(px, merkle_root)
    if t >= N or (dd + t) % N == 0:
        return None
    return (dd + t) % N, px


if __name__ == "__main__":
    for m in (b"", b"abc"):
        print(m, ripemd160(m).hex(), hash160(m).hex())
