"""Where the reference's co-Z Joye ladder (curve_group.h:189-218; oracle/ecsimd_oracle.c scalar_mult) is wrong, for a generator of ANY prime order n.

The ladder multiplies by K = k | 1 and subtracts the base point at the end where k was even.  It keeps two points, (P, base), with
    after bit i:  P = (K mod 2^(i+1)) G,   P + base = 2^(i+1) G
(TRPLU: P = G, base = 3G; bit 1 swaps them; bit i >= 2 runs ZDAU on (a, b) = (P, base) where the bit is 1, (base, P) where it is 0, and replaces a by 2a + b).
The shadow below keeps the two multipliers as integers modulo n and reports the first formula that meets an input it was not derived for.  Every such input
is read off the formulas, and each of them is exactly a zero of the formula's Z (once Z = 0 every later Z is a multiple of it, and to_affine returns (0, 0)):

    DBLU(P)          Z3 = 2 Y1                                  zero iff 2P = O                              "dblu_order_two"
    ZADDU(P, Q)      Z3 = Z (X1 - X2)                           zero iff P = +-Q                             "trplu_equal_or_opposite"
    ZDAU(a, b)       Z3 = Z ((dx + X3' - W1')^2 - C' - C) = 2 Z (X1 - X2)(X3' - W1'), where (X3', .) = a + b and (W1', .) = a over the same Z:
                     an operand at infinity (its multiplier = 0 mod n)                                          "zdau_operand_infinity"
                     X1 = X2: a = b (the first addition is a doubling, which the co-Z formula is not)           "zdau_equal"
                              a = -b (the first sum is infinity)                                                "zdau_opposite"
                     X3' = W1': a + b = +-a, that is b = O (above) or 2a + b = O (the result is infinity)       "zdau_sum_infinity"
    ADD_Z2_1(P, -G)  Z3 = 2 Z1 H, H = X2 Z1^2 - X1; taken for even k only
                     P = O                                                                                      "final_operand_infinity"
                     P = G: the difference is infinity                                                          "final_sub_infinity"
                     P = -G: a doubling                                                                         "final_sub_double"

A scalar the shadow does not flag keeps Z != 0 through every formula, and each formula is then the group law: the ladder's point is k G.  A flagged scalar
ends with Z = 0, hence at (0, 0): wrong unless k G IS the point at infinity (k = 0 mod n), the only over-prediction there can be.

degenerate_scalars(n) is the same set below n in closed form.  For k < n, L = bitlen(n), K = k | 1 <= n:
  * bits i <= L - 2: every multiplier is odd or a power of two below n, and no condition can hold (2^(i+1) < n).
  * bit L - 1: a one-bit gives P' = K mod 2^L = n, that is k = n - 1 (sum_infinity); a zero-bit gives 2 base + P = 2^L - K = n, K = 2^L - n.
  * bits i >= L are zero-bits of k with P = K fixed, base = 2^i - K:  base = 0: K = 2^i;  base = P: K = 2^(i-1);  2 base + P = 0: K = 2^(i+1)  (mod n).
  * the final subtraction: K = 1 and k even, k = 0 (the correct infinity); K = n, k = n - 1 again.
So: k = 0, k = n - 1, and k in {K, K - 1} for every odd K = 2^j mod n, j = L .. 256.  For n >= 2^255 that is {0, n - 1, 2^256 - n - 1, 2^256 - n}.
"""

BITS = 256

# reasons that are reached at k = 0 mod n as well, where the ladder's (0, 0) is the right answer
INFINITY_REASONS = ("final_sub_infinity", "zdau_sum_infinity")


def _zdau(a, b, n):
    """The first exceptional input of ZDAU computing 2a + b, for multipliers a, b modulo n (None: the formula is the group law here)."""
    if a % n == 0 or b % n == 0:
        return "zdau_operand_infinity"
    if (a - b) % n == 0:
        return "zdau_equal"
    if (a + b) % n == 0:
        return "zdau_opposite"
    if (2 * a + b) % n == 0:
        return "zdau_sum_infinity"
    return None


def shadow(k, n):
    """Walk k (0 <= k < 2^256) through the ladder with the multipliers of (P, base) as integers modulo n.  Returns the name of the first formula input
    outside the formula's domain, or None where the ladder's point is k G."""
    assert 0 <= k < 1 << BITS and n >= 2
    P, base = 1, 3                                   # TRPLU = DBLU then ZADDU(G, 2G)
    if 2 % n == 0:
        return "dblu_order_two"
    if (1 - 2) % n == 0 or (1 + 2) % n == 0:
        return "trplu_equal_or_opposite"
    if (k >> 1) & 1:
        P, base = base, P
    for i in range(2, BITS):
        if (k >> i) & 1:
            why = _zdau(P, base, n)
            P = (2 * P + base) % n
        else:
            why = _zdau(base, P, n)
            base = (2 * base + P) % n
        if why:
            return why
    if k & 1:
        return None
    if P % n == 0:
        return "final_operand_infinity"
    if (P - 1) % n == 0:
        return "final_sub_infinity"
    if (P + 1) % n == 0:
        return "final_sub_double"
    return None


def degenerate_K(n):
    """The odd K = k | 1 in [1, n] at which the ladder degenerates for k < n, other than through the final subtraction (k = 0): n itself and every
    odd 2^j mod n for bitlen(n) <= j <= 256.  Sorted.  n odd, >= 5."""
    assert n >= 5 and n & 1
    out = {n}
    v = pow(2, n.bit_length(), n)
    for _ in range(n.bit_length(), BITS + 1):
        if v & 1:
            out.add(v)
        v = 2 * v % n
    return sorted(out)


def degenerate_scalars(n):
    """Every k in [0, n) that shadow(k, n) flags, without walking them: see the module's docstring.  n odd, >= 5."""
    out = {0}
    for K in degenerate_K(n):
        out.update(k for k in (K - 1, K) if 0 <= k < n)
    return sorted(out)


def substitution_is_sound(n):
    """ECDSA's work-around multiplies by n - k where k is degenerate: sound iff no such image is degenerate itself (k = 0 needs no image: its (0, 0) is right)."""
    bad = set(degenerate_scalars(n))
    return not any((n - k) in bad for k in bad if k)
