#!/usr/bin/env python3
"""Host model of BIP-32 key derivation: SHA-512 in plain Python, HMAC-SHA-512, the master key of a seed, CKDpriv, CKDpub and a path of them, on Python integers.

What ecsimd_hip_sha512, _hmac_sha512, _bip32_master, _bip32_ckd_priv and _bip32_ckd_pub promise, written down once without any of the library's code.  The
compression function is here for the two "Bitcoin seed" midstates the device source holds as literals; its constants are not typed in but computed, as
FIPS 180-4 defines them: the first 64 bits of the fractional parts of the square roots (initial state) and cube roots (round constants) of the first primes.
sha512 and hmac_sha512 below are built on it and held to `hashlib` / `hmac` by tests/test_bip32_cpu.py, which also pins the model to the published BIP-32
test vectors (tests/golden/bip32_vectors.json).  The curve arithmetic comes from tools/bip340_model.py.

Integers in and out: a key or a chain code is the big-endian reading of its 32 bytes.  A refused input gives None.
"""
import hashlib
import hmac as _hmac
from math import isqrt

from bip340_model import GX, GY, N, P, add, mul_g   # noqa: F401

HARDENED = 1 << 31
SEED_KEY = b"Bitcoin seed"
_M64 = (1 << 64) - 1


def _icbrt(v):
    lo, hi = 0, 1 << ((v.bit_length() + 2) // 3 + 1)
    while lo < hi:
        mid = (lo + hi + 1) // 2
        if mid ** 3 <= v:
            lo = mid
        else:
            hi = mid - 1
    return lo


def _primes(count):
    out, c = [], 2
    while len(out) < count:
        if all(c % q for q in out):
            out.append(c)
        c += 1
    return out


K = [_icbrt(q << 192) & _M64 for q in _primes(80)]
IV = [isqrt(q << 128) & _M64 for q in _primes(8)]


def _rotr(x, n):
    return ((x >> n) | (x << (64 - n))) & _M64


def compress(state, block):
    """One 128-byte block into a state of eight 64-bit words; returns the new state."""
    assert len(block) == 128 and len(state) == 8
    w = [int.from_bytes(block[8 * i:8 * i + 8], "big") for i in range(16)]
    for t in range(16, 80):
        s0 = _rotr(w[t - 15], 1) ^ _rotr(w[t - 15], 8) ^ (w[t - 15] >> 7)
        s1 = _rotr(w[t - 2], 19) ^ _rotr(w[t - 2], 61) ^ (w[t - 2] >> 6)
        w.append((w[t - 16] + s0 + w[t - 7] + s1) & _M64)
    a, b, c, d, e, f, g, h = state
    for t in range(80):
        t1 = (h + (_rotr(e, 14) ^ _rotr(e, 18) ^ _rotr(e, 41)) + ((e & f) ^ (~e & g & _M64)) + K[t] + w[t]) & _M64
        t2 = ((_rotr(a, 28) ^ _rotr(a, 34) ^ _rotr(a, 39)) + ((a & b) ^ (a & c) ^ (b & c))) & _M64
        a, b, c, d, e, f, g, h = (t1 + t2) & _M64, a, b, c, (d + t1) & _M64, e, f, g
    return [(x + y) & _M64 for x, y in zip(state, (a, b, c, d, e, f, g, h))]


def finish(state, data, prefix_bytes=0):
    """The digest of a hash whose first prefix_bytes bytes (a multiple of 128) are in `state` already and whose rest is `data`."""
    padded = data + b"\x80" + b"\x00" * ((111 - len(data)) % 128) + (8 * (prefix_bytes + len(data))).to_bytes(16, "big")
    for i in range(0, len(padded), 128):
        state = compress(state, padded[i:i + 128])
    return b"".join(x.to_bytes(8, "big") for x in state)


def sha512(msg):
    return finish(IV, msg)


def hmac_midstates(key):
    """(inner, outer): the states after the key's ipad block and after its opad block (RFC 2104; a key of more than 128 bytes is hashed first)."""
    if len(key) > 128:
        key = sha512(key)
    block = key + bytes(128 - len(key))
    return compress(IV, bytes(b ^ 0x36 for b in block)), compress(IV, bytes(b ^ 0x5c for b in block))


def hmac_sha512(key, msg):
    inner, outer = hmac_midstates(key)
    return finish(outer, finish(inner, msg, 128), 128)


def _b(x):
    return x.to_bytes(32, "big")


def ser_p(pt):
    return bytes([2 | (pt[1] & 1)]) + _b(pt[0])


def master(seed):
    """(k, c) of the seed, or None where IL = 0 or IL >= n."""
    i = hmac_sha512(SEED_KEY, seed)
    k = int.from_bytes(i[:32], "big")
    return None if k == 0 or k >= N else (k, int.from_bytes(i[32:], "big"))


def ckd_priv(k, c, index):
    """(k_child, c_child), or None where k is outside [1, n - 1], IL >= n or the child key is 0."""
    if not 1 <= k < N:
        return None
    data = (b"\x00" + _b(k) if index >= HARDENED else ser_p(mul_g(k))) + index.to_bytes(4, "big")
    i = hmac_sha512(_b(c), data)
    il = int.from_bytes(i[:32], "big")
    child = (il + k) % N
    return None if il >= N or child == 0 else (child, int.from_bytes(i[32:], "big"))


def on_curve(x, y):
    return 0 <= x < P and 0 <= y < P and (y * y - x * x * x - 7) % P == 0


def ckd_pub(pt, c, index):
    """((x, y), c_child), or None for a hardened index, a point off the curve, IL >= n or an infinite sum."""
    if index >= HARDENED or not on_curve(*pt):
        return None
    i = hmac_sha512(_b(c), ser_p(pt) + index.to_bytes(4, "big"))
    il = int.from_bytes(i[:32], "big")
    if il >= N:
        return None
    q = add(pt, mul_g(il)) if il else pt
    return None if q is None else (q, int.from_bytes(i[32:], "big"))


def derive(k, c, path):
    """(k, c) at the end of `path` (a list of indices) below (k, c), or None where a level refuses."""
    for index in path:
        node = ckd_priv(k, c, index)
        if node is None:
            return None
        k, c = node
    return k, c


def fingerprint(k):
    """The first four bytes of HASH160(serP(k G)): what a child's serialization calls its parent."""
    from btc_model import hash160
    return hash160(ser_p(mul_g(k)))[:4]


if __name__ == "__main__":
    assert sha512(b"abc") == hashlib.sha512(b"abc").digest() and hmac_sha512(b"k", b"m") == _hmac.new(b"k", b"m", hashlib.sha512).digest()
    for name, mid in zip(("inner", "outer"), hmac_midstates(SEED_KEY)):
        print(name, ", ".join("0x%016xull" % x for x in mid))
