"""Curves whose generator has a prime order n < 2^255, for the tests of the ladder route of ECDSA on a registered curve (tools/ladder_degenerate_model.py):

  * textbook affine arithmetic on Python integers (None = infinity),
  * tiny curves generated from a seed, their order counted with a table of quadratic residues,
  * NIST P-192 (FIPS 186-4 D.1.2.1),
  * curves y^2 = x^3 + b with a prime order of a chosen bit length, constructed by complex multiplication with j = 0:
    `python tools/short_order_curves.py` prints the fixture tests/golden/short_order_curves.json.

Every curve has p = 3 mod 4 and p < 2n, which is what ecsimd_hip_register_curve asks before it grants ECDSA.
"""
import random


def affine_model(c):
    p, a = c["p"], c["a"]

    def add(P, Q):
        if P is None: return Q
        if Q is None: return P
        (x1, y1), (x2, y2) = P, Q
        if x1 == x2:
            if (y1 + y2) % p == 0: return None
            lam = (3 * x1 * x1 + a) * pow(2 * y1, -1, p) % p
        else:
            lam = (y2 - y1) * pow(x2 - x1, -1, p) % p
        x3 = (lam * lam - x1 - x2) % p
        return x3, (lam * (x1 - x3) - y1) % p

    def mul(k, P):
        R = None
        for bit in bin(k)[2:] if k else "":
            R = add(R, R)
            if bit == "1": R = add(R, P)
        return R
    return add, mul


def is_prime(n):
    if n < 2: return False
    for q in (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37):
        if n % q == 0: return n == q
    d, r = n - 1, 0
    while d % 2 == 0:
        d //= 2; r += 1
    for a in (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37):        # deterministic below 3.3e24, a strong probable-prime test above
        x = pow(a, d, n)
        if x in (1, n - 1): continue
        for _ in range(r - 1):
            x = x * x % n
            if x == n - 1: break
        else:
            return False
    return True


def validate(c):
    """What a fixture must satisfy, in the Python model: p = 3 mod 4, G on the curve, n prime, n G = O, p < 2n."""
    p, a, b, n = c["p"], c["a"], c["b"], c["n"]
    G = (c["gx"], c["gy"])
    _, mul = affine_model(c)
    assert p % 4 == 3 and is_prime(p) and (4 * a ** 3 + 27 * b * b) % p
    assert (G[1] ** 2 - G[0] ** 3 - a * G[0] - b) % p == 0 and G[1]
    assert is_prime(n) and p < 2 * n and mul(n, G) is None
    return True


P192 = dict(p=2 ** 192 - 2 ** 64 - 1, a=2 ** 192 - 2 ** 64 - 4, b=0x64210519e59c80e70fa7e9ab72243049feb8deecc146b9b1,
            gx=0x188da80eb03090f67cbf20eb43a18800f4ff0afd82ff1012, gy=0x07192b95ffc8da78631011ed6b24cdd573f977a11e794811,
            n=0xffffffffffffffffffffffff99def836146bc9b1b4d22831)


# ---------------------------------------------------------------- tiny curves
def count_points(p, a, b):
    """#E(GF(p)) with a table of squares: 1 + sum over x of (1 + chi(x^3 + a x + b))."""
    roots = [0] * p
    for y in range(p):
        roots[y * y % p] += 1
    return 1 + sum(roots[(x * x * x + a * x + b) % p] for x in range(p))


def tiny_curve(bits, a_kind, seed):
    """The first curve of the seeded stream with a prime p = 3 mod 4 of `bits` bits and a prime number n of points (then every point but O generates, and
    p < 2n by Hasse for p >= 2^6).  a_kind: "0", "-3" or "random"."""
    rng = random.Random(seed)
    while True:
        p = rng.getrandbits(bits) | (1 << (bits - 1)) | 3
        if not is_prime(p) or (a_kind == "0" and p % 3 != 1):     # a = 0, p = 2 mod 3: supersingular, p + 1 points
            continue
        for _ in range(64):
            a = {"random": rng.randrange(1, p), "-3": p - 3, "0": 0}[a_kind]
            b = rng.randrange(1, p)
            if (4 * a ** 3 + 27 * b * b) % p == 0:
                continue
            n = count_points(p, a, b)
            if not is_prime(n) or p >= 2 * n:
                continue
            for x in range(p):
                rhs = (x ** 3 + a * x + b) % p
                y = pow(rhs, (p + 1) // 4, p)
                if y and y * y % p == rhs:
                    return dict(p=p, a=a, b=b, gx=x, gy=y, n=n)


TINY = [(7, "0", 7001), (8, "-3", 8001), (9, "random", 9001), (10, "0", 10001), (11, "-3", 11001), (13, "random", 13001)]     # (bits of p, a, seed)


def tiny_curves():
    return {"tiny%d_a%s" % (bits, kind): tiny_curve(bits, kind, seed) for bits, kind, seed in TINY}


# ---------------------------------------------------------------- complex multiplication, j = 0
def cornacchia_3(p):
    """(t, s) with 4p = t^2 + 3 s^2 for a prime p = 7 mod 12: x^2 + 3 y^2 = p by Cornacchia, then t = 2x, s = 2y."""
    import math
    r = pow(p - 3, (p + 1) // 4, p)                               # a square root of -3 (p = 3 mod 4; -3 is a square as p = 1 mod 3)
    assert (r * r + 3) % p == 0
    if 2 * r < p: r = p - r
    a_, b_ = p, r
    lim = math.isqrt(p)
    while b_ > lim:
        a_, b_ = b_, a_ % b_
    y2, rem = divmod(p - b_ * b_, 3)
    y = math.isqrt(y2)
    assert rem == 0 and y * y == y2
    return 2 * b_, 2 * y


def cm_curve(pbits, order_bits, cofactor, seed):
    """y^2 = x^3 + b over a prime p = 7 mod 12 of `pbits` bits with a generator of prime order n of `order_bits` bits, p < 2n: the six orders of the
    twists of j = 0 are p + 1 +- t and p + 1 +- (t +- 3s) / 2, and one of them must be cofactor * n.  (p < 2n and Hasse leave cofactor 1, or cofactor 2 on
    a curve with more than p points.)"""
    rng = random.Random(seed)
    while True:
        p = rng.getrandbits(pbits) | (1 << (pbits - 1))
        p -= (p - 7) % 12
        if p.bit_length() != pbits or not is_prime(p):
            continue
        t, s = cornacchia_3(p)
        assert t * t + 3 * s * s == 4 * p
        cands = [p + 1 + t, p + 1 - t] + [p + 1 + sg * (t + sh * 3 * s) // 2 for sg in (1, -1) for sh in (1, -1)]
        goal = [m for m in cands if m % cofactor == 0 and (m // cofactor).bit_length() == order_bits and p < 2 * (m // cofactor) and is_prime(m // cofactor)]
        if not goal:
            continue
        n = goal[0] // cofactor
        for b in range(1, 400):
            _, mul = affine_model(dict(p=p, a=0, b=b))
            for x in range(1, 50):
                rhs = (x ** 3 + b) % p
                y = pow(rhs, (p + 1) // 4, p)
                if not y or y * y % p != rhs:
                    continue
                R = (x, y)
                if mul(goal[0], R) is None and all(mul(m, R) is not None for m in cands if m != goal[0]):
                    G = mul(cofactor, R)
                    if G is not None:
                        return dict(p=p, a=0, b=b, gx=G[0], gy=G[1], n=n)
                break                                             # this b is another twist: the next one


# name: (bits of p, bits of n, cofactor, seed).  What cannot be had: a 256-bit p with its top bit set and an order below 2^255 that keeps p < 2n needs
# cofactor 2 (n > p / 2 >= 2^254, n < 2^255), and j = 0 has none -- with p = x^2 + 3 y^2 the even twist orders are p + 1 +- 2x = (x +- 1)^2 + 3 y^2, always
# multiples of 4, and the other four are odd (the search for (256, 255, 2) ran dry accordingly); an order of 224 bits under such a p breaks p < 2n outright.
# So the fixtures have p of the order's own size: 255 bits (every 32-bit word and all nine 29-bit limbs in use) and 224 bits (a generic short order: about
# half of the 2^j mod n are odd).
CM = {"cm255": (255, 255, 1, 255001), "cm224": (224, 224, 1, 224001)}


if __name__ == "__main__":
    import json
    import sys
    out = {}
    for name, args in CM.items():
        c = cm_curve(*args)
        validate(c)
        out[name] = {k: format(v, "x") for k, v in c.items()}
    json.dump(out, sys.stdout, indent=1)
    sys.stdout.write("\n")
