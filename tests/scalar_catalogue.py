"""The scalars at which the window loops' recodings can go wrong, one list per built-in curve, with the reason each one is there.

catalogue(cv) -> [(k, {feature names})], at most 400 scalars, pure Python.  tests/test_recoding_models.py proves the conditions the list is built
to meet; tests/test_gpu_scalar_routes.py runs it through every variable-base and fixed-base route on the device.

Both curves: the edge lists of the GPU parity tests (restated here: they are local to those tests), the combs' exceptional scalars, a thin
sample of the digit-pattern family (24 of the 16 796 scalars the windowed tests run, every 700th), the ladder's three degenerate scalars
(`ladder_degenerate`) and k = 0 mod n (`zero_mod_n`).

secp256k1 in addition: scalars built for the GLV split of k_varwin.inc, k = k1 + k2 lambda.  GlvWordModel restates the split as the kernels do it --
32-bit words, the rounding bit added to word 12 of the product with a carry chain over four words, 256-bit two's-complement differences of low
products, abs256 word by word, the + 0x88..8 offset, 33 nibbles under an unsigned top one -- so that a scalar can be AIMED at one link of those chains:

  carry_g<i>_w<j>   round(k g_i / 2^384) carries out of j all-ones low words: k = ceil((2m + 1) 2^383 / g_i), m = h 2^(32 j) + 2^(32 j) - 1
  k1_zero, k2_zero  one half is zero (every one of its digits is skipped)
  sign_pp .. sign_nn   the four sign pairs (zero counts as positive, as in abs256)
  top1_half1, top1_half2   the unsigned top digit is 1: |half| >= 0x7777..78.  (Both at once cannot happen: the split's cell reaches 0.4625 x 2^128 in
                    both halves at best, below 0x7777..78 = 0.4667 x 2^128 -- tests/test_recoding_models.py proves it; `top1_both` stays a name with no scalar.)
  neg_borrow_w<j>   a negative half whose magnitude has exactly j zero low words: abs256's borrow starts at word j
  digit_<d>_everywhere   all 32 signed 4-bit digits of a half, the half's sign applied, are d (d = -8 .. 8; 8 is the negative half of 0x77..78).  The sign is part of it: a magnitude with raw
                    digit -5 .. -1 everywhere would be 2^128 - |d| 0x11..1 > 0.66 x 2^128, outside the cell; the negative half of |d| 0x11..1 adds -|d| P everywhere
  lattice           lambda, the basis vectors and their neighbours (the list of test_windowed_variable_base_matches_the_ladder_at_affine_level)

For every secp256k1 scalar the module asserts, when the catalogue is built: the word model equals the integer formula, |k1|, |k2| < 2^128, the digits
sum to the halves, and k1 + k2 lambda = k (mod n)."""
from helpers import CURVE_PARAMS, P256, SECP256K1

M32 = (1 << 32) - 1
M256 = (1 << 256) - 1
LAMBDA = 0x5363ad4cc05c30e0a5261c028812645a122e22ea20816678df02967c1b23bd72
G1 = 0x3086d221a7d46bcde86c90e49284eb153daa8a1471e8ca7fe893209a45dbb031
G2 = 0xe4437ed6010e88286f547fa90abfe4c4221208ac9df506c61571b4ae8ac47f71
A1, MB1, A2 = 0x3086d221a7d46bcde86c90e49284eb15, 0xe4437ed6010e88286f547fa90abfe4c3, 0x114ca50f7a8e2f3f657c1108d9d44cfd8
TOP1 = int("7" * 31 + "8", 16)            # the smallest magnitude whose top digit is 1: 2^128 - 0x88..8
ONES = int("1" * 32, 16)
CARRY_HIGH = (0, 1, 0x1234567)            # the part of c above the all-ones words


def words(v, count=8):
    return [(v >> (32 * i)) & M32 for i in range(count)]


def unwords(w):
    return sum(x << (32 * i) for i, x in enumerate(w))


def signed256(v):
    v &= M256
    return v - (1 << 256) if v >> 255 else v


def glv_split_integers(k):
    """The formula of test_glv_split_of_secp256k1 on Python integers, k already below n: (k1, k2) signed."""
    c1 = ((k * G1) >> 384) + (((k * G1) >> 383) & 1)
    c2 = ((k * G2) >> 384) + (((k * G2) >> 383) & 1)
    return signed256(k - ((c1 * A1) & M256) - ((c2 * A2) & M256)), signed256(((c1 * MB1) & M256) - ((c2 * A1) & M256))


class GlvWordModel:
    """k_varwin_mult_glv / k_varwin_mult_glv_ct up to the digits, on lists of 32-bit words.  cut_carry: the deliberately wrong rounding whose carry
    stops after word 0 -- the fault the carry_* scalars exist to expose (tests/test_recoding_models.py holds the model to that)."""

    def __init__(self, cut_carry=False):
        self.cut_carry = cut_carry

    @staticmethod
    def mul8x8(a, b):
        t = [0] * 16
        for i in range(8):
            carry = 0
            for j in range(8):
                s = t[i + j] + a[i] * b[j] + carry
                t[i + j] = s & M32; carry = s >> 32
            t[i + 8] = carry
        return t

    @staticmethod
    def sub8(a, b):
        out, borrow = [], 0
        for x, y in zip(a, b):
            d = x - y - borrow
            out.append(d & M32); borrow = 1 if d < 0 else 0
        return out, borrow

    @staticmethod
    def add8(a, b):
        out, carry = [], 0
        for x, y in zip(a, b):
            s = x + y + carry
            out.append(s & M32); carry = s >> 32
        return out

    def round_shift_384(self, k, g):
        t = self.mul8x8(k, words(g))
        c = t[12:16]
        carry = t[11] >> 31                                # v_add_co_u32, then three v_addc_co_u32
        for i in range(4):
            s = c[i] + carry
            c[i] = s & M32; carry = s >> 32
            if self.cut_carry and i == 0:
                carry = 0
        return c + [0, 0, 0, 0]

    def low_product(self, a, b):
        return self.mul8x8(a, b)[:8]

    def abs256(self, v):
        neg = v[7] >> 31
        m, _ = self.sub8([0] * 8, v)
        return (m if neg else v), neg

    def split(self, k):
        """k < 2^256 -> (k1, k2) signed, and per half (sign, [digit_0 .. digit_31, top digit], as digit_of returns them before the sign)."""
        n = CURVE_PARAMS[SECP256K1]["n"]
        kk = words(k)
        d, borrow = self.sub8(kk, words(n))
        kk = kk if borrow else d
        c1, c2 = self.round_shift_384(kk, G1), self.round_shift_384(kk, G2)
        t, _ = self.sub8(kk, self.low_product(c1, words(A1)))
        k1, _ = self.sub8(t, self.low_product(c2, words(A2)))
        k2, _ = self.sub8(self.low_product(c1, words(MB1)), self.low_product(c2, words(A1)))
        halves = []
        for v in (k1, k2):
            mag, neg = self.abs256(v)
            u = self.add8(mag, [0x88888888] * 4 + [0] * 4)[:5]                      # the loops keep five words
            nib = [(u[j // 8] >> (4 * (j % 8))) & 15 for j in range(33)]
            halves.append((neg, [x - 8 for x in nib[:32]] + [nib[32]], unwords(mag)))
        return signed256(unwords(k1)), signed256(unwords(k2)), halves


WORD_MODEL = GlvWordModel()


def checked_split(k):
    """The word model's split of k, held to the integer formula and to the identities the loops rely on."""
    n = CURVE_PARAMS[SECP256K1]["n"]
    k1, k2, halves = WORD_MODEL.split(k)
    assert (k1, k2) == glv_split_integers(k % n), hex(k)
    assert abs(k1) < 1 << 128 and abs(k2) < 1 << 128 and (k1 + k2 * LAMBDA - k) % n == 0, hex(k)
    for v, (neg, digits, mag) in zip((k1, k2), halves):
        assert mag == abs(v) and neg == (1 if v < 0 else 0) and digits[32] in (0, 1) and all(-8 <= x < 8 for x in digits[:32]), hex(k)
        assert sum(x << (4 * j) for j, x in enumerate(digits)) == mag, hex(k)
    return k1, k2, halves


def carry_scalars():
    """[(k, 'carry_g<i>_w<j>')]: c = floor(k g / 2^384) ends in j all-ones words and bit 383 of k g is set, so the rounding carries through them."""
    n = CURVE_PARAMS[SECP256K1]["n"]
    out = []
    for gi, g in ((1, G1), (2, G2)):
        for w in (1, 2, 3):
            for h in CARRY_HIGH:
                m = (h << (32 * w)) | ((1 << (32 * w)) - 1)
                k = -(-((2 * m + 1) << 383) // g)
                if (k * g) >> 384 == m and ((k * g) >> 383) & 1 and k < n:
                    out.append((k, "carry_g%d_w%d" % (gi, w)))
                    if k + n <= M256:
                        out.append((k + n, "carry_g%d_w%d" % (gi, w)))
    return out


def digit_magnitude(d):
    """The magnitude whose 32 low digits are all d: d 0x11..1, under a top digit of 1 for a negative d."""
    return d * ONES if d >= 0 else (1 << 128) + d * ONES


def chosen_halves():
    """(k1, k2) aimed at the recoding's edges, kept only where the split returns exactly that pair (its cell is a parallelogram)."""
    n = CURVE_PARAMS[SECP256K1]["n"]
    mags = [0, 1, 7, 8, 9, 1 << 32, (1 << 32) - 1, 1 << 64, (1 << 64) - 1, 1 << 96, (1 << 96) - 1, TOP1 - 1, TOP1, ONES, 8 * ONES, (1 << 124) - 1, 1 << 127]
    mags += [digit_magnitude(d) for d in range(-8, 8) if digit_magnitude(d) not in mags]
    # partners for the other half: zero, a small odd value and two of no particular shape, one of them next to the top digit's threshold
    partners = [0, 0x5a5a5a5a5a5a5a5a1d, 0x2b992ddfa23249d6c3a5f08e1b7c9d4f, TOP1 + 0x1234567]
    pairs = []
    for m in mags:
        for q in partners:
            for s1 in (1, -1):
                for s2 in (1, -1):
                    pairs += [(s1 * m, s2 * q), (s1 * q, s2 * m)]
    out, seen = [], set()
    for k1, k2 in pairs:
        k = (k1 + k2 * LAMBDA) % n
        if k in seen or k == 0:
            continue
        seen.add(k)
        if glv_split_integers(k) == (k1, k2):
            out.append(k)
    return out


def glv_features(k):
    k1, k2, halves = checked_split(k)
    f = set()
    if k1 == 0: f.add("k1_zero")
    if k2 == 0: f.add("k2_zero")
    f.add("sign_" + ("n" if k1 < 0 else "p") + ("n" if k2 < 0 else "p"))
    t1, t2 = halves[0][1][32], halves[1][1][32]
    if t1 and t2: f.add("top1_both")
    elif t1: f.add("top1_half1")
    elif t2: f.add("top1_half2")
    for neg, digits, mag in halves:
        if neg:
            zeros = next(j for j in range(8) if (mag >> (32 * j)) & M32)
            if zeros in (1, 2, 3): f.add("neg_borrow_w%d" % zeros)
        signed = {(-x if neg else x) for x in digits[:32]}
        if len(signed) == 1:
            f.add("digit_%d_everywhere" % signed.pop())
    return f


def lattice_scalars():
    n = CURVE_PARAMS[SECP256K1]["n"]
    lam = LAMBDA
    return [lam, lam + 1, lam - 1, (2 * lam) % n, n - lam, (lam * lam) % n, A1, A1 + 1, A1 - 1, MB1, MB1 + 8, A2, A2 - 8, (A1 * lam) % n,
            (MB1 * lam) % n, (A1 + MB1 * lam) % n, (8 + 8 * lam) % n, (n - 8 - 8 * lam) % n, (1 << 128) - 1, 1 << 128, ((1 << 128) * lam) % n,
            (((1 << 128) - 1) * (lam + 1)) % n, (0x88888888888888888888888888888888 * (lam + 1)) % n]


def comb_exceptional_scalars(cv):
    """tests/test_gpu_parity.py comb_exceptional_scalars (the GPU file holds this copy to it)."""
    n = CURVE_PARAMS[cv]["n"]
    out = []
    for low_bits in (4, 20 * 12, 7 * 36, 5 * 51, 6 * 42, 20, 7, 249):
        m = n % (1 << low_bits)
        out += [n - 2 * m, (2 * m) % n, n - 2 * m + 1, n - 2 * m - 1]
    out += [v + n for v in out if v + n < (1 << 256)]
    return [v for v in out if v % n != 0]


PATTERN_WORDS = (0, 1, 0x7fffffff, 0x80000000, 0xfffffffe, 0xffffffff)
PATTERN_STEP = 100 * 700                  # the windowed tests run every 100th operand of the family; every 700th of those


def digit_pattern_sample():
    """Rows 0, 70 000, 140 000, .. of test_oracle.digit_pattern_operands() (6^8 rows; the row number's base-6 digits, most significant first, choose
    the 32-bit words from the least significant up), as integers."""
    out = []
    for r in range(0, 6 ** 8, PATTERN_STEP):
        idx = [(r // 6 ** (7 - j)) % 6 for j in range(8)]
        out.append(unwords([PATTERN_WORDS[i] for i in idx]))
    return out


def edge_scalars(cv):
    """The union of the edge lists of test_scalar_mult_vs_oracle, test_windowed_variable_base_matches_the_ladder_at_affine_level (without its lattice part)
    and test_small_base_batches_take_the_comb_and_keep_the_ladders_bits."""
    order = CURVE_PARAMS[cv]["n"]
    a = [0, 1, 2, 3, 4, 5, 6, 7, 8, order - 2, order - 1, order, order + 1, order + 2, 2**256 - 1, 2**256 - 2, 2**255, 2**255 - 1,
         2**64, 2**64 - 1, 2**128, 2**192 + 1, int("55" * 32, 16), int("aa" * 32, 16), 2**256 - order, 2**256 - order - 1, 2**256 - order + 1]
    b = [0, order, 1, 2, 7, 8, 9, 15, 16, 17, 0x78, 0x80, 0x88, 2**252, 2**255, (order - 1) // 2, (order + 1) // 2, order - 2, order - 1,
         order + 1, order + 9, 2**256 - 1, 2**256 - order, 2**256 - order - 1, int("8" * 64, 16), int("7" * 64, 16), int("9" * 64, 16),
         int("08" * 32, 16), int("80" * 32, 16), int("f0" * 32, 16), int("0f" * 32, 16)]
    c = [0, 1, 2, 3, order - 2, order - 1, order, order + 1, 2**256 - order - 2, 2**256 - order - 1, 2**256 - order, 2**256 - order + 1,
         2**256 - 1, 2**255, 2**255 - 1, (order - 1) // 2, (order + 1) // 2, 2 * order - 2**256, 31, 32, 2**5 - 1, 2**250]
    return a + b + c


def ladder_degenerate_scalars(cv):
    """The co-Z ladder's point is not k P at these (tools/ladder_degenerate_model.py): n - 1 and the two scalars that meet n P at the last step."""
    order = CURVE_PARAMS[cv]["n"]
    return {order - 1, 2**256 - order, 2**256 - order - 1}


HALVES_PER_FEATURE = 6
_CACHE = {}


def catalogue(cv):
    if cv in _CACHE:
        return _CACHE[cv]
    order = CURVE_PARAMS[cv]["n"]
    feats = {}

    def add(k, *names):
        assert 0 <= k <= M256
        feats.setdefault(k, set()).update(names)
    for k in edge_scalars(cv): add(k, "edge")
    for k in comb_exceptional_scalars(cv): add(k, "comb_exceptional")
    for k in digit_pattern_sample(): add(k, "digit_pattern")
    if cv == SECP256K1:
        for k in lattice_scalars(): add(k, "lattice")
        for k, name in carry_scalars(): add(k, name)
        # the chosen halves, thinned: a pair is kept while one of its features has fewer than HALVES_PER_FEATURE scalars
        count = {}
        for k in chosen_halves():
            f = glv_features(k)
            if any(count.get(name, 0) < HALVES_PER_FEATURE for name in f):
                add(k, "chosen_halves")
                for name in f: count[name] = count.get(name, 0) + 1
    for k in list(feats):
        if k in ladder_degenerate_scalars(cv): feats[k].add("ladder_degenerate")
        if k % order == 0: feats[k].add("zero_mod_n")
        if cv == SECP256K1: feats[k] |= glv_features(k)
    _CACHE[cv] = [(k, frozenset(f)) for k, f in feats.items()]
    return _CACHE[cv]


def with_feature(cv, *prefixes):
    """The catalogue's scalars that carry a feature starting with one of the prefixes, in catalogue order."""
    return [k for k, f in catalogue(cv) if any(name.startswith(p) for name in f for p in prefixes)]
