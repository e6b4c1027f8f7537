"""The input batches of tests/test_gpu_msm_schedule.py and the conditions they are built to meet -- shared with tests/test_msm_cases_cpu.py, which holds every
generator to its condition and to the schedule of tools/msm_model.py without a GPU.  Expected values are NOT made here: both tests take them from the big-int
group law of tests/helpers.py.

Four families:
  WIDTH_CASES        every window width c = 1 .. 16 at the smallest n that gives it, distinct random scalars on distinct points: every bucket populated.
  one_hot_batches    one non-zero digit per scalar, in every window, with the bit patterns a digit extractor gets wrong: aimed at the windows that straddle a
                     32-bit word.
  layout_batches     bits = c (or 2 c): the count of each digit fixes every bucket's [a, b) in `sorted`, and the counts are drawn so that a bucket begins and
                     ends on, before and behind the edges of the slices: all 17 classes of layout_class.
  order_edge_scalars the scalars around the group order.

A plain module, not a conftest: nothing here is collected.
"""
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
if ROOT not in sys.path: sys.path.insert(0, ROOT)
import msm_model as model  # noqa: E402
from helpers import CURVE_PARAMS, P256, SECP256K1, ec_add  # noqa: E402

CURVES = (P256, SECP256K1)
AUTO, BUCKETS, LANES = model.ALG_AUTO, model.ALG_BUCKETS, model.ALG_LANES
WALK = 4099
MASK64 = (1 << 64) - 1


def G(cv):
    return (CURVE_PARAMS[cv]["gx"], CURVE_PARAMS[cv]["gy"])


_walks = {}


def walk(cv):
    """P_i = (i + 1) G for i < 4099, by repeated addition: computed once per curve and never changed."""
    if cv not in _walks:
        P, out = G(cv), []
        for _ in range(WALK):
            out.append(P); P = ec_add(cv, P, G(cv))
        _walks[cv] = tuple(out)
    return _walks[cv]


def limbs_of(vals):
    """Python integers below 2^256 -> (n, 4) uint64, little-endian limbs."""
    vals = list(vals)
    if not vals: return np.zeros((0, 4), dtype=np.uint64)
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in vals), dtype="<u8").reshape(len(vals), 4).copy()


def ints_of(arr):
    """(n, 4) uint64 -> Python integers."""
    raw = np.ascontiguousarray(arr, dtype="<u8").tobytes()
    return [int.from_bytes(raw[32 * i:32 * i + 32], "little") for i in range(len(arr))]


def tree_passes(plan):
    return model.tree_passes(plan["buckets"] // plan["m"])


# ---------------------------------------------------------------- 1. every window width on populated buckets
# (c, n, windows, m, L, per_window, tree passes) as the issue tabulated them; the CPU test holds the model to these rows, the GPU test the library.
WIDTH_TABLE = (
    (7, 2048, 37, 16, 16, 8, 1),
    (9, 8192, 29, 32, 32, 16, 1),
    (11, 32768, 24, 32, 64, 64, 2),
    (13, 131072, 20, 32, 128, 256, 2),
    (14, 262144, 19, 32, 128, 512, 3),
    (16, 1048576, 16, 32, 256, 2048, 3),
)
# (c, n, bits): n = 2^(c + 4) is the smallest n at which the planner gives c (c <= floor(log2 n) - 4); c = 1 needs bits = 1.
WIDTH_CASES = ((1, 64, 1),) + tuple((c, 1 << (c + 4), 256) for c in range(2, 17))
# a partial top window behind a width that straddles the words: both values of bits keep c = 7, 9, 11, 13 at these sizes
PARTIAL_TOP_CASES = tuple((c, 1 << (c + 4), bits) for c in (7, 9, 11, 13) for bits in (255, 129))
LANES_MAX_N = 1 << 20                   # LANES runs beside BUCKETS up to here
SPOT_LANES = 64                         # lanes of the device's a_i G compared with the big-int product, per case


def width_case_id(case):
    return "c%d-n%d-bits%d" % case


def width_batch(cv, n, bits):
    """(a, k): a = n distinct random 63-bit multipliers of G as uint64 (n,), k = n distinct scalars of 256 random bits as uint64 (n, 4).  The bits of k above
    `bits` are NOT cleared: the device has to."""
    rng = np.random.default_rng([0x6d736d, cv, n, bits])
    a = rng.integers(1, 1 << 63, size=n, dtype=np.uint64)
    k = rng.integers(0, 1 << 64, size=(n, 4), dtype=np.uint64, endpoint=False)
    return a, k


def mask_limbs(k, bits):
    """k mod 2^bits on (n, 4) uint64."""
    out = k.copy()
    for j in range(4):
        lo = 64 * j
        if bits <= lo: out[:, j] = 0
        elif bits < lo + 64: out[:, j] &= np.uint64((1 << (bits - lo)) - 1)
    return out


def dot_mod(k, a, bits, order):
    """sum (k_i mod 2^bits) a_i mod order, exactly: the four limb columns and a as Python integers."""
    km = mask_limbs(k, bits)
    ao = a.astype(object)
    total = 0
    for j in range(4):
        if km[:, j].any(): total += int((km[:, j].astype(object) * ao).sum()) << (64 * j)
    return total % order


# ---------------------------------------------------------------- 2. one-hot windows at the word boundaries
ONE_HOT_WIDTHS = (3, 5, 7, 9, 11, 13)
ONE_HOT_BITS = (256, 255)
PATTERNS = ("one", "all ones", "top bit", "below the top bit", "alternating", "random")


def straddling_windows(c, windows):
    """The windows whose c bits lie in two 32-bit words."""
    return [w for w in range(windows) if (w * c) % 32 + c > 32]


def digit_pattern(name, c, rng):
    if name == "one": return 1
    if name == "all ones": return (1 << c) - 1
    if name == "top bit": return 1 << (c - 1)
    if name == "below the top bit": return (1 << (c - 1)) - 1
    if name == "alternating": return sum(1 << j for j in range(c - 1, -1, -2))      # 0b1010...: the top bit set
    return rng.randrange(1, 1 << c)


def one_hot_rounds(n, windows):
    """Batches per case: term i's window is i mod windows, so a window meets n // windows terms of one batch; where that is below the number of patterns (c = 3:
    128 terms over 86 windows) the batch is repeated with the patterns rotated, until every window has met every pattern."""
    return 1 if n // windows >= len(PATTERNS) else len(PATTERNS)


def one_hot_batches(c, n, bits):
    """[(scalars, tags)]: scalars[i] < 2^256 has ONE non-zero c-bit digit, in window i mod windows (cut at 2^256 where the top window reaches beyond; the bits at
    and above `bits` are left for the device to drop); tags[i] = (window, pattern name, digit)."""
    plan = model.plan(n, bits, BUCKETS)
    assert plan["c"] == c
    W = plan["windows"]
    out = []
    for r in range(one_hot_rounds(n, W)):
        rng = random.Random("one hot / %d %d %d %d" % (c, n, bits, r))
        ks, tags = [], []
        for i in range(n):
            w, name = i % W, PATTERNS[(i // W + r) % len(PATTERNS)]
            d = digit_pattern(name, c, rng)
            ks.append((d << (w * c)) & ((1 << 256) - 1)); tags.append((w, name, d))
        out.append((ks, tags))
    return out


# ---------------------------------------------------------------- 3. every layout of a bucket over the slices
# (n, bits): c = 4, one window, L = 4 / c = 4, two windows, L = 8, the second window begins inside a slice / c = 8, one window, L = 32
LAYOUT_SHAPES = ((256, 4), (257, 8), (4099, 8))
LAYOUT_BATCHES = 64
LAYOUT_LANES_BATCHES = 4                # LANES runs beside BUCKETS on the first four batches of a shape
LAYOUT_CLASSES = 17


def layout_class(a, b, L):
    """The structural class of a bucket at sorted[a, b) under slices of L entries: "empty", or (spans, a on a slice edge, b on a slice edge, slices wholly
    covered between the first and the last it touches: 0, 1 or 2 for two and more; always 0 inside one slice).  17 classes."""
    if a == b: return "empty"
    s0, s1 = a // L, (b - 1) // L
    return (s0 != s1, a % L == 0, b % L == 0, min(2, max(0, s1 - s0 - 1)))


def all_layout_classes():
    inside = {(False, ae, be, 0) for ae in (False, True) for be in (False, True)}
    spans = {(True, ae, be, mid) for ae in (False, True) for be in (False, True) for mid in (0, 1, 2)}
    return {"empty"} | inside | spans


def digit_counts(rng, n, c, L):
    """How many of n terms have each digit 0 .. 2^c - 1: digit 0 shifts the alignment, the others are lengths around the multiples of L, one absorbs the rest."""
    counts = [0] * (1 << c)
    counts[0] = rng.choice((0, 1, 2, 3, L))
    menu = (0, 1, L - 1, L, L + 1, 2 * L - 1, 2 * L, 2 * L + 1, 3 * L, 3 * L + 1, 4 * L)
    others = list(range(1, 1 << c))
    rng.shuffle(others)
    absorber, left = others[0], n - counts[0]
    for d in others[1:]:
        counts[d] = min(rng.choice(menu), left)
        left -= counts[d]
    counts[absorber] = left
    assert sum(counts) == n and min(counts) >= 0
    return counts


def layout_batch(n, bits, index):
    """(scalars, counts): counts[w][d] terms have digit d in window w, drawn independently per window and shuffled over the terms independently."""
    plan = model.plan(n, bits, BUCKETS)
    c, W, L = plan["c"], plan["windows"], plan["L"]
    rng = random.Random("layout / %d %d %d" % (n, bits, index))
    ks, counts = [0] * n, []
    for w in range(W):
        cnt = digit_counts(rng, n, c, L)
        digits = [d for d, m in enumerate(cnt) for _ in range(m)]
        rng.shuffle(digits)
        for i, d in enumerate(digits): ks[i] |= d << (w * c)
        counts.append(cnt)
    return ks, counts


def bucket_ranges(n, counts):
    """[(window, digit, a, b)] for every bucket (digit != 0): window w owns sorted[w n, (w + 1) n), grouped by ascending digit, digit 0 in front."""
    out = []
    for w, cnt in enumerate(counts):
        a = w * n
        for d, m in enumerate(cnt):
            if d: out.append((w, d, a, a + m))
            a += m
        assert a == (w + 1) * n
    return out


def layout_classes_of(n, bits, counts):
    L = model.plan(n, bits, BUCKETS)["L"]
    return {layout_class(a, b, L) for _, _, a, b in bucket_ranges(n, counts)}


# ---------------------------------------------------------------- 4. LANES across a product chunk
CHUNK_N, CHUNK_BITS = (1 << 22) + 17, 64


def chunk_scalars():
    """One random 64-bit word in the low limb, random bits in the other three: bits = 64 must ignore them."""
    return np.random.default_rng(0x4c414e45).integers(0, 1 << 64, size=(CHUNK_N, 4), dtype=np.uint64, endpoint=False)


def chunk_dot(k, order):
    """sum k_i[0] ((i mod 4099) + 1) mod order: the low limbs are summed per residue first, in 32-bit halves so that no uint64 wraps."""
    low = k[:, 0]
    pad = (-len(low)) % WALK
    halves = []
    for half in (low & np.uint64(0xffffffff), low >> np.uint64(32)):
        halves.append(np.concatenate([half, np.zeros(pad, dtype=np.uint64)]).reshape(-1, WALK).sum(axis=0, dtype=np.uint64))
    assert (len(low) + pad) // WALK < 1 << 32
    return sum((int(lo) + (int(hi) << 32)) * (r + 1) for r, (lo, hi) in enumerate(zip(*halves))) % order


# ---------------------------------------------------------------- 5. operands nobody has passed yet
def sqrt_b(cv):
    """y with y^2 = b, or None where b is no square mod p (p = 3 mod 4 on both curves)."""
    p, b = CURVE_PARAMS[cv]["p"], CURVE_PARAMS[cv]["b"]
    assert p % 4 == 3
    y = pow(b, (p + 1) // 4, p)
    return y if y * y % p == b else None


def order_edge_scalars(cv):
    order = CURVE_PARAMS[cv]["n"]
    return (order - 1, order, order + 1, 2 * order % (1 << 256), (1 << 256) - 1)
