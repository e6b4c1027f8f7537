#!/usr/bin/env python3
"""Host model of deterministic ECDSA nonces (RFC 6979 section 3.2 with HMAC-SHA-256) on Python integers, `hmac` and `hashlib` only.

What ecsimd_hip_rfc6979_nonce and ecsimd_hip_ecdsa_sign_deterministic promise, written down once without any of the library's code, so that the
expected values of the GPU tests do not rest on the code under test.  Supported where qlen = 256 (the group order n >= 2^255): no bit shifts, h1 is the
32 big-endian bytes of e, bits2octets(h1) is e - n where e >= n, int2octets(d) the 32 big-endian bytes of d.  e is any 256-bit value; the result is
RFC 6979 proper when e is a SHA-256 digest (another 256-bit digest: what libsecp256k1 does).  tests/test_ecdsa_deterministic_cpu.py pins this model to
the known answers of RFC 6979 A.2.5.
"""
import hashlib
import hmac
import math


def digest_int(message):
    """SHA-256(message) as the integer the ECDSA calls take."""
    return int.from_bytes(hashlib.sha256(message).digest(), "big")


def candidates_needed(n):
    """C(n): the least C with (1 - n / 2^256)^C <= 2^-128 -- how many candidates a caller must be able to try for a failure to be that unlikely.
    Evaluated in double precision, as the library does when it looks a curve up: ceil(128 / -log2(1 - n / 2^256)).  (SM2's 2^256 - n is 2^224 (1 + 2^-96.9):
    the quotient rounds to 2^-32 and C = 4, where exact arithmetic would ask for a fifth candidate to cover an excess of one part in 2^95 over 2^-128.)"""
    return math.ceil(128 / -math.log2(((1 << 256) - n) / (1 << 256)))


def nonce(n, e, d, cap=None):
    """(k, rejected): the nonce for digest e and private key d and the number of candidates step h.3 rejected before it.
    None where d is outside [1, n - 1] or `cap` candidates were all rejected."""
    if n < 1 << 255 or n >= 1 << 256:
        raise ValueError("qlen = 256 only")
    if not 1 <= d < n:
        return None
    x = d.to_bytes(32, "big")
    h1 = (e - n if e >= n else e).to_bytes(32, "big")
    mac = lambda key, msg: hmac.new(key, msg, hashlib.sha256).digest()
    V, K = b"\x01" * 32, b"\x00" * 32          # b, c
    K = mac(K, V + b"\x00" + x + h1)          # d
    V = mac(K, V)                              # e
    K = mac(K, V + b"\x01" + x + h1)          # f
    V = mac(K, V)                              # g
    rejected = 0
    while cap is None or rejected < cap:
        V = mac(K, V)                          # h.2: one HMAC gives the 256 bits
        k = int.from_bytes(V, "big")
        if 1 <= k < n:
            return k, rejected
        rejected += 1
        K = mac(K, V + b"\x00")                # h.3
        V = mac(K, V)
    return None


def sign(c, e, d, low_s=False, cap=None):
    """(r, s, v, k) of the deterministic signature on curve c (a dict with p, a, b, gx, gy, n), or None where the call refuses the lane.
    One deviation from RFC 6979, the library's: r = 0 or s = 0 refuses the lane instead of drawing the next candidate."""
    from ecdsa_recover_model import sign_recoverable
    kn = nonce(c["n"], e, d, cap)
    if kn is None:
        return None
    sig = sign_recoverable(c, e, d, kn[0], low_s=low_s)
    return None if sig is None else (*sig, kn[0])
