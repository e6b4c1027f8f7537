#!/usr/bin/env python3
"""Host model of ECDSA public-key recovery and of the recovery id (SEC 1 v2 4.1.6), on plain Python integers.

What ecsimd_hip_ecdsa_recover and ecsimd_hip_ecdsa_sign_recoverable promise, written down once without any of the library's code, so that the expected
values of the GPU tests do not rest on the code under test.  A curve is a dict with p, a, b, gx, gy, n (tests/helpers.py CURVE_PARAMS, ecsimd_amd.curves.NAMED);
p = 3 mod 4.  Points are (x, y) tuples, None is the point at infinity.  tests/test_ecdsa_recover_cpu.py checks this model against the textbook ec_mul.
"""


def ec_add(c, P, Q):
    p = c["p"]
    if P is None:
        return Q
    if Q is None:
        return P
    x1, y1 = P
    x2, y2 = Q
    if x1 == x2:
        if (y1 + y2) % p == 0:
            return None
        lam = (3 * x1 * x1 + c["a"]) * pow(2 * y1, -1, p) % p
    else:
        lam = (y2 - y1) * pow(x2 - x1, -1, p) % p
    x3 = (lam * lam - x1 - x2) % p
    return x3, (lam * (x1 - x3) - y1) % p


def ec_mul(c, k, P):
    acc = None
    while k:
        if k & 1:
            acc = ec_add(c, acc, P)
        P = ec_add(c, P, P)
        k >>= 1
    return acc


def is_square(c, x):
    """x^3 + a x + b is a square modulo p (zero included): Euler's criterion."""
    p = c["p"]
    rhs = (x * x * x + c["a"] * x + c["b"]) % p
    return rhs == 0 or pow(rhs, (p - 1) // 2, p) == 1


def lift(c, r, v):
    """R = (r + (v >> 1) n, the root with parity v & 1), or None where v > 3, x >= p, x is not on the curve, or that root does not exist."""
    p = c["p"]
    x = r + (v >> 1) * c["n"]
    if v > 3 or x >= p or x >= 1 << 256:
        return None
    rhs = (x * x * x + c["a"] * x + c["b"]) % p
    y = pow(rhs, (p + 1) // 4, p)
    if y * y % p != rhs:
        return None
    if (y ^ v) & 1:
        if y == 0:
            return None
        y = p - y
    return x, y


def front_end(c, e, r, s, v):
    """(valid, u1, u2, R): what the device's front end hands to the double-scalar sum.  Invalid elements get u1 = u2 = 0 and R = G."""
    n = c["n"]
    R = lift(c, r, v) if 1 <= r < n and 1 <= s < n else None
    if R is None:
        return False, 0, 0, (c["gx"], c["gy"])
    w = pow(r, -1, n)
    return True, (n - e * w) % n, s * w % n, R


def recover(c, e, r, s, v):
    """Q = (-e / r) G + (s / r) R, or None where the element is refused or Q is the point at infinity."""
    valid, u1, u2, R = front_end(c, e, r, s, v)
    if not valid:
        return None
    return ec_add(c, ec_mul(c, u1, (c["gx"], c["gy"])), ec_mul(c, u2, R))


def sign_recoverable(c, e, d, k, low_s=False, kG=None):
    """(r, s, v) of the textbook signature with the nonce k, or None where ecdsa_sign refuses (d, k out of range, r = 0 or s = 0).  kG: k G from somewhere else."""
    n = c["n"]
    if not (1 <= d < n and 1 <= k < n):
        return None
    x, y = kG if kG is not None else ec_mul(c, k, (c["gx"], c["gy"]))
    r = x % n
    s = pow(k, -1, n) * (e + r * d) % n
    if r == 0 or s == 0:
        return None
    v = (y & 1) | (2 if x >= n else 0)
    if low_s and s > n // 2:
        s, v = n - s, v ^ 1
    return r, s, v



def chain_of_existing_calls(engine, curve, order_field, c, e, r, s, v):
    """The same recovery chained from the engine's OTHER public calls, every intermediate through device memory: the bit-for-bit oracle of
    tests/test_gpu_ecdsa_recover.py and the timing baseline of tools/bench_kernels.py.  e, r, s: (n, 4) device tensors, v: uint8 device tensor.
    Returns (qx, qy, finite, x_fits) as the calls leave them -- the chain checks NO range and no square: lanes that ecdsa_recover refuses hold
    whatever the calls make of them (double_scalar_mult still refuses a point that is not on the curve), and the caller masks them."""
    import numpy as np
    n = e.shape[0]
    limbs = lambda value: np.tile(np.array([[(value >> (64 * i)) & (2**64 - 1) for i in range(4)]], dtype=np.uint64), (n, 1))
    order, zero = engine.to_device(limbs(c["n"])), engine.to_device(limbs(0))
    w = engine.mgry_to_classical(order_field, engine.gfp_inverse(order_field, engine.mgry_from_classical(order_field, r)))      # 1 / r mod n
    u1 = engine.gfp_opposite(order_field, engine.mod_mul(order_field, engine.sub_if_above(e, order), w))                        # -e / r
    u2 = engine.mod_mul(order_field, s, w)                                                                                      # s / r
    x, carry = engine.add(r, engine.if_else(((v >> 1) & 1).contiguous(), order, zero))                                          # r + j n
    y, _ = engine.compute_y(curve, x)
    flip = engine.mask_op(0, engine.mask_op(3, engine.mask_bit(y, 0), (v & 1).contiguous()))                                    # parity(y) != v & 1
    y = engine.if_else(flip, engine.gfp_opposite(curve, y), y)
    qx, qy, finite = engine.double_scalar_mult(curve, u1, u2, x, y)
    return qx, qy, finite, engine.mask_op(0, carry)

if __name__ == "__main__":
    import random
    c = dict(p=0xfffffffffffffffffffffffffffffffffffffffffffffffffffffffefffffc2f, a=0, b=7,
             gx=0x79be667ef9dcbbac55a06295ce870b07029bfcdb2dce28d959f2815b16f81798, gy=0x483ada7726a3c4655da4fbfc0e1108a8fd17b448a68554199c47d08ffb10d4b8,
             n=0xfffffffffffffffffffffffffffffffebaaedce6af48a03bbfd25e8cd0364141)
    rng = random.Random(1)
    for _ in range(8):
        e, d, k = rng.getrandbits(256), rng.randrange(1, c["n"]), rng.randrange(1, c["n"])
        r, s, v = sign_recoverable(c, e, d, k, low_s=True)
        assert recover(c, e, r, s, v) == ec_mul(c, d, (c["gx"], c["gy"])) and s <= c["n"] // 2
    print("ecdsa_recover_model: 8 secp256k1 round trips ok")
