#!/usr/bin/env python3
"""Host models of the kernels that decide, after a hash, whether the hash is usable as a scalar modulo the group order -- with the order as a PARAMETER.

One function per kernel of k_bip32.hip, k_schnorr.hip, k_btc.hip (the Taproot part), k_recover.hip (the recovery id) and per order-dependent helper of ECDSA
(ecdsa_sign_scalars, x_mod_n_equals), restating the contract the kernel's header comment gives: `hashlib` / `hmac` and Python integers, nothing of the library's
code.  Every function takes the order n first and states EVERY output of the lane, what a refused lane holds included.  Where a kernel takes a point as input
arrays (the affine d G, k G, ...) the model takes the same integers and uses them as given: there is no curve arithmetic here but the even-y lift of an
x-only key, which the public front kernels do themselves.  p and G are secp256k1's: the kernels have them compiled in, only n is an argument.

An order here is what the kernels assume of one: odd and 2^255 < n < 2^256, so that a 256-bit value is below 2 n and one subtraction reduces it.
tests/test_launch_tails_cpu.py holds these models, at the real order, to tools/bip32_model.py, bip340_model.py, btc_model.py, ecdsa_recover_model.py and the
published vectors; tests/test_gpu_launch_tails.py holds the kernels to them at orders that put many lanes on the refused side.
"""
import functools
import hashlib
import hmac

P = 0xfffffffffffffffffffffffffffffffffffffffffffffffffffffffefffffc2f
N = 0xfffffffffffffffffffffffffffffffebaaedce6af48a03bbfd25e8cd0364141
GX = 0x79be667ef9dcbbac55a06295ce870b07029bfcdb2dce28d959f2815b16f81798
GY = 0x483ada7726a3c4655da4fbfc0e1108a8fd17b448a68554199c47d08ffb10d4b8
HARDENED = 1 << 31
_2_256 = 1 << 256


def check_order(n):
    assert n & 1 and 1 << 255 < n < _2_256, "an order the kernels can take: odd, 2^255 < n < 2^256"


def _b(x):
    return x.to_bytes(32, "big")


def _int(b):
    return int.from_bytes(b, "big")


def tagged(tag, data):
    t = hashlib.sha256(tag.encode()).digest()
    return _int(hashlib.sha256(t + t + data).digest())


@functools.lru_cache(maxsize=None)         # (a pure function of px: the batches ask for the same lifts at every order)
def lift_even(px):
    """The point with that x and an even y, or None (px >= p, or x^3 + 7 is not a square)."""
    if px >= P:
        return None
    c = (pow(px, 3, P) + 7) % P
    y = pow(c, (P + 1) // 4, P)
    if y * y % P != c:
        return None
    return px, (y if y % 2 == 0 else P - y)


def on_curve(x, y):
    return x < P and y < P and (y * y - x * x * x - 7) % P == 0


# ---- k_bip32.hip
def master_digest(seed):
    i = hmac.new(b"Bitcoin seed", seed, hashlib.sha512).digest()
    return _int(i[:32]), _int(i[32:])


def bip32_master(n, seed):
    """(k, c, ok): zeros where IL = 0 or IL >= n."""
    il, ir = master_digest(seed)
    return (il, ir, 1) if 1 <= il < n else (0, 0, 0)


def ckd_digest(c_par, prefix, x, index):
    i = hmac.new(_b(c_par), bytes([prefix]) + _b(x) + index.to_bytes(4, "big"), hashlib.sha512).digest()
    return _int(i[:32]), _int(i[32:])


def ckd_priv_digest(k_par, c_par, index, point):
    """(IL, IR) of CKDpriv as the kernel forms its data: 00 || k_par for a hardened index, serP of the given point otherwise (point None: the kernel without
    point arrays, which hashes 00 || k_par whatever the index and refuses the lane where it is not hardened)."""
    if index >= HARDENED or point is None:
        return ckd_digest(c_par, 0, k_par, index)
    return ckd_digest(c_par, 2 | (point[1] & 1), point[0], index)


def bip32_ckd_priv(n, k_par, c_par, index, point):
    """(k_child, c_child, ok): zeros where k_par is not in [1, n - 1], IL >= n, k_child = 0, or (point None) the index is not hardened."""
    if not 1 <= k_par < n or (point is None and index < HARDENED):
        return 0, 0, 0
    il, ir = ckd_priv_digest(k_par, c_par, index, point)
    child = (il + k_par) % n
    return (0, 0, 0) if il >= n or child == 0 else (child, ir, 1)


def ckd_pub_digest(qx, qy, c_par, index):
    return ckd_digest(c_par, 2 | (qy & 1), qx, index)


def bip32_ckd_pub_front(n, qx, qy, c_par, index):
    """(x, y, t, c_child, valid): K, IL, IR where the index is not hardened, K is on the curve and IL < n; G, 0, 0 and valid = 0 where not."""
    il, ir = ckd_pub_digest(qx, qy, c_par, index)
    if index < HARDENED and on_curve(qx, qy) and il < n:
        return qx, qy, il, ir, 1
    return GX, GY, 0, 0, 0


def bip32_ckd_pub_accept(ax, ay, jz, valid, c_child):
    """(cx, cy, c_child, ok): the affine sum and the chain code kept where valid and Z != 0, zeros where not."""
    return (ax, ay, c_child, 1) if valid != 0 and jz != 0 else (0, 0, 0, 0)


# ---- k_schnorr.hip
def challenge_digest(r, px, msg):
    return tagged("BIP0340/challenge", _b(r) + _b(px) + msg)


def schnorr_verify_front(n, px, r, s, msg):
    """(u1, u2, x, y, valid): s, n - e (0 staying 0), the even-y lift of px where it exists and r < p and s < n; 0, 0, G and valid = 0 where not."""
    e = challenge_digest(r, px, msg) % n
    pt = lift_even(px)
    if pt is None or r >= P or s >= n:
        return 0, 0, GX, GY, 0
    return s, (n - e) % n, pt[0], pt[1], 1


def nonce_digest(n, d, aux, px, py, msg):
    """int(H_nonce(t || px || m)); aux None: 32 zero bytes.  (Only a d in [1, n - 1] has a nonce; for another d this is a hash of 256 bits that nothing uses.)"""
    dd = (n - d) % _2_256 if py & 1 else d
    t = dd ^ tagged("BIP0340/aux", _b(aux or 0))
    return tagged("BIP0340/nonce", _b(t) + _b(px) + msg)


def schnorr_nonce(n, d, aux, px, py, msg):
    """k0: the nonce hash modulo n, 0 where d is not in [1, n - 1]."""
    return nonce_digest(n, d, aux, px, py, msg) % n if 1 <= d < n else 0


def schnorr_finish(n, d, k0, xP, yP, xR, yR, msg):
    """(px, r, s, ok) for 0 <= k0 < n: zeros where k0 = 0; else r = xR, s = k + e d' with k = k0 or n - k0 by the parity of yR, d' = d or n - d by that of yP."""
    if k0 == 0:
        return 0, 0, 0, 0
    e = challenge_digest(xR, xP, msg) % n
    dd = ((n - d) % _2_256 if yP & 1 else d) % n
    k = n - k0 if yR & 1 else k0
    return xP, xR, (k + e * dd) % n, 1


# ---- k_btc.hip
def tap_tweak(px, merkle):
    return tagged("TapTweak", _b(px) + (b"" if merkle is None else _b(merkle)))


def tweak_front(n, px, merkle):
    """(x, y, t, valid) of the hashed modes (merkle None: key path): the even-y lift and t where it exists and t < n; G, 0 and valid = 0 where not."""
    t = tap_tweak(px, merkle)
    pt = lift_even(px)
    return (pt[0], pt[1], t, 1) if pt is not None and t < n else (GX, GY, 0, 0)


def taproot_seckey(n, d, merkle, xP, yP):
    """(d_out, px, ok): d' + t mod n and xP; zeros where d is not in [1, n - 1], t >= n or the sum is 0."""
    t = tap_tweak(xP, merkle)
    if not 1 <= d < n or t >= n:
        return 0, 0, 0
    out = ((n - d if yP & 1 else d) + t) % n
    return (out, xP, 1) if out else (0, 0, 0)


# ---- k_recover.hip, k_gfield.hip, k_affine.inc / k_gcurve.hip
def sign_recovery_id(n, x, y, s, ok, low_s):
    """(s, v): v = parity(y) | (x >= n ? 2 : 0), 0 where ok = 0; with low_s, s > n / 2 becomes n - s and flips bit 0 of v."""
    v = (y & 1) | (2 if x >= n else 0)
    if low_s and s > n // 2:
        s, v = n - s, v ^ 1
    return s, (v if ok else 0)


def ecdsa_sign_scalars(n, e, d, k, x):
    """(r, s, ok) for x < 2 n and a prime n: r = x mod n, s = (e + r d) / k; zeros where d or k is not in [1, n - 1], r = 0 or s = 0."""
    if not (1 <= d < n and 1 <= k < n):
        return 0, 0, 0
    r = x - n if x >= n else x
    s = pow(k, -1, n) * (e + r * d) % n
    return (r, s, 1) if r and s else (0, 0, 0)


def x_mod_n_equals(n, x, finite, r):
    """ok = finite and x mod n == r, for x < 2 n."""
    return int(finite != 0 and (x - n if x >= n else x) == r)
