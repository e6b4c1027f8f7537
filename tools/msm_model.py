"""The host model of ecsimd_msm (include/ecsimd_msm.h; ecsimd_amd/csrc/msm_stages.cuh, k_msm.inc): the schedule of ecsimd_msm_plan restated in Python -- the same c, L, m,
launches and workspace from the same (n, bits, flags) -- and an index-level emulation of the BUCKETS route's stages on Python integers: digits and
validation, the counting sort by (window, digit), the slices with their head / tail slots, the combination of a bucket's slices, the bucket reduction in
chunks, the tree sum and the Horner step over the windows.  Every virtual lane counts the point operations (additions and doublings) it performs one after the
other, so the serial bound of the header (max_chain) is checked on adversarial batches and not merely asserted.

The group law here is the textbook affine one on integers (None = the point at infinity): the emulation follows the device's INDICES, not its coordinates."""

ALG_AUTO, ALG_BUCKETS, ALG_LANES = 0, 1, 2
MAX_N = 1 << 24
AUTO_THRESHOLD = 1 << 20
TREE_FAN = 16
VARWIN_CHUNK = 1 << 22

P256, SECP256K1 = 0, 1
CURVES = {
    P256: dict(p=0xffffffff00000001000000000000000000000000ffffffffffffffffffffffff, a=-3,
               b=0x5ac635d8aa3a93e7b3ebbd55769886bc651d06b0cc53b0f63bce3c3e27d2604b,
               gx=0x6b17d1f2e12c4247f8bce6e563a440f277037d812deb33a0f4a13945d898c296,
               gy=0x4fe342e2fe1a7f9b8ee7eb4a7c0f9e162bce33576b315ececbb6406837bf51f5,
               n=0xffffffff00000000ffffffffffffffffbce6faada7179e84f3b9cac2fc632551),
    SECP256K1: dict(p=0xfffffffffffffffffffffffffffffffffffffffffffffffffffffffefffffc2f, a=0, b=7,
                    gx=0x79be667ef9dcbbac55a06295ce870b07029bfcdb2dce28d959f2815b16f81798,
                    gy=0x483ada7726a3c4655da4fbfc0e1108a8fd17b448a68554199c47d08ffb10d4b8,
                    n=0xfffffffffffffffffffffffffffffffebaaedce6af48a03bbfd25e8cd0364141),
}


# ---------------------------------------------------------------- the schedule (capi.hip msm_schedule_of, msm_carve)
def floor_log2(v):
    return v.bit_length() - 1 if v > 0 else 0


def ceil_log2(v):
    return 0 if v <= 1 else (v - 1).bit_length()


def ceil_div(a, b):
    return (a + b - 1) // b


def tree_passes(count):
    p = 0
    while count > 1:
        count = ceil_div(count, TREE_FAN)
        p += 1
    return p


def round16(b):
    return ceil_div(b, 16) * 16


def varwin_scratch_bytes(n):
    return n * (7 * 4 * 32 + 8 * 64)


def schedule(n, bits=256, flags=ALG_AUTO):
    """Everything the host derives from (n, bits, flags): the plan's fields and the internal sizes.  ValueError where ecsimd_msm_plan returns BAD_ARG."""
    if not 1 <= bits <= 256 or not 0 <= n <= MAX_N or flags not in (ALG_AUTO, ALG_BUCKETS, ALG_LANES):
        raise ValueError((n, bits, flags))
    S = dict(route=flags if flags != ALG_AUTO else (ALG_BUCKETS if n >= AUTO_THRESHOLD else ALG_LANES), c=0, windows=0, buckets=0, L=0, m=0, max_chain=0,
             launches=0, workspace_bytes=0, T=0, K=0, slices=0, per_window=0, chunk_lanes=0, front_lanes=0)
    if n == 0:
        S["launches"] = 1
        return S
    if S["route"] == ALG_BUCKETS:
        c = min(bits, min(16, max(2, floor_log2(n) - 4)))
        windows = ceil_div(bits, c)
        c = ceil_div(bits, windows)                           # the same number of windows, evenly wide
        buckets = 1 << c
        L = max(4, (1 << ((ceil_log2(n) + 1) // 2)) // 4)
        m = min(buckets, max(2, min(32, 1 << ((c + 1) // 2))))
        T, K = n * windows, windows << c
        slices, per_window = ceil_div(T, L), buckets // m
        chunk_lanes = per_window * windows
        S.update(c=c, windows=windows, buckets=buckets, L=L, m=m, T=T, K=K, slices=slices, per_window=per_window, chunk_lanes=chunk_lanes,
                 max_chain=max(L, ceil_div(n, L) + 1, 2 * m + 2 * c, TREE_FAN, windows * (c + 1)), launches=8 + tree_passes(per_window))
        S["workspace_bytes"] = (round16(16 + 4 * K) + round16(4 * (K + 1)) + round16(4 * K) + round16(4 * T) + 3 * 32 * n + 32 * 3 * K + 32 * 3 * 2 * slices
                                + 32 * 3 * chunk_lanes)
    else:
        front = ceil_div(n, TREE_FAN)
        S.update(front_lanes=front, max_chain=TREE_FAN, launches=4 + 5 * ceil_div(n, VARWIN_CHUNK) + tree_passes(front))
        S["workspace_bytes"] = 32 + 5 * 32 * n + 32 * 3 * front + varwin_scratch_bytes(min(n, VARWIN_CHUNK))
    return S


PLAN_FIELDS = ("route", "c", "windows", "buckets", "L", "m", "max_chain", "launches", "workspace_bytes")


def plan(n, bits=256, flags=ALG_AUTO):
    """ecsimd_msm_plan_t as a dict."""
    S = schedule(n, bits, flags)
    return {f: S[f] for f in PLAN_FIELDS}


# ---------------------------------------------------------------- the group law on integers
def ec_add(cv, P, Q):
    c = CURVES[cv]; p = c["p"]
    if P is None: return Q
    if Q is None: return P
    x1, y1 = P; x2, y2 = Q
    if x1 == x2:
        if (y1 + y2) % p == 0: return None
        lam = (3 * x1 * x1 + c["a"]) * pow(2 * y1, -1, p) % p
    else:
        lam = (y2 - y1) * pow(x2 - x1, -1, p) % p
    x3 = (lam * lam - x1 - x2) % p
    return x3, (lam * (x1 - x3) - y1) % p


def ec_mul(cv, k, P):
    R, Q = None, P
    while k:
        if k & 1: R = ec_add(cv, R, Q)
        Q = ec_add(cv, Q, Q); k >>= 1
    return R


def classify(cv, pt):
    """0 infinity, 1 a point of the curve, 2 invalid -- k_msm.inc classify."""
    c = CURVES[cv]; p = c["p"]
    x, y = pt
    if x == 0 and y == 0: return 0
    return 1 if (x < p and y < p and (y * y - (x * x * x + c["a"] * x + c["b"])) % p == 0) else 2


class Lane:
    """One virtual lane: counts the point operations it executes one after the other."""
    def __init__(self, cv): self.cv, self.ops = cv, 0
    def add(self, P, Q): self.ops += 1; return ec_add(self.cv, P, Q)
    def dbl(self, P): self.ops += 1; return ec_add(self.cv, P, P)


def tree_sum(cv, arr, stats):
    """k_msm_tree on one group: lanes own strided slices of TREE_FAN elements, one pass per launch, down to one element."""
    count = len(arr)
    while count > 1:
        lanes = ceil_div(count, TREE_FAN)
        for g in range(lanes):
            ln = Lane(cv); acc = arr[g]
            for t in range(1, TREE_FAN):
                e = g + t * lanes
                if e >= count: break
                acc = ln.add(acc, arr[e])
            arr[g] = acc
            stats["tree"] = max(stats.get("tree", 0), ln.ops)
        count = lanes
    return arr[0]


def msm_buckets(cv, ks, pts, bits=256, order=None):
    """The BUCKETS route index by index.  ks: ints; pts: (x, y) ints, (0, 0) = infinity.  order: the permutation inside a bucket that the scatter's atomics
    happened to give -- any function from a list of term indices to a reordering of it (None: ascending).  Returns (the affine sum or None, invalid, stats) with
    stats[stage] = the largest number of point operations one lane of that stage performed."""
    n = len(ks)
    S = schedule(n, bits, ALG_BUCKETS)
    stats = {}
    if n == 0: return None, 0, stats
    c, W, L, m, T, K = S["c"], S["windows"], S["L"], S["m"], S["T"], S["K"]
    dmask = (1 << c) - 1
    # 1. digits and validation
    cls = [classify(cv, pt) for pt in pts]
    invalid = sum(1 for v in cls if v == 2)
    kk = [(k & ((1 << bits) - 1)) if v == 1 else 0 for k, v in zip(ks, cls)]
    digit = lambda i, w: (kk[i] >> (w * c)) & dmask
    # 2. histogram, scan, scatter: every term has one entry per window, digit 0 included
    hist = [0] * K
    for i in range(n):
        for w in range(W): hist[(w << c) + digit(i, w)] += 1
    start = [0] * (K + 1)
    for key in range(K): start[key + 1] = start[key] + hist[key]
    assert start[K] == T
    members = [[] for _ in range(K)]
    for i in range(n):
        for w in range(W): members[(w << c) + digit(i, w)].append(i)
    srt = []
    for key in range(K): srt.extend(order(members[key]) if order else members[key])
    assert len(srt) == T and all(start[(w << c)] == w * n for w in range(W))
    # 3. slices
    slices = S["slices"]
    bucket, partial = {}, {}
    for s in range(slices):
        ln = Lane(cv)
        p0, p1 = s * L, min(s * L + L, T)
        state = dict(cur=None, acc=None, first=p0)
        def flush():
            key = state["cur"]
            if key is None or key & dmask == 0: return
            if start[key] >= p0 and start[key + 1] <= p1: assert key not in bucket; bucket[key] = state["acc"]
            else: slot = 2 * s + (0 if state["first"] == p0 else 1); assert slot not in partial; partial[slot] = state["acc"]
        for pos in range(p0, p1):
            w = pos // n
            idx = srt[pos]; d = digit(idx, w); key = (w << c) + d
            if key != state["cur"]:
                flush(); state.update(cur=key, acc=None, first=pos)
            if d: state["acc"] = ln.add(state["acc"], pts[idx])
        flush()
        stats["slices"] = max(stats.get("slices", 0), ln.ops)
    # ... and the buckets that span slices
    for key in range(K):
        if key & dmask == 0: continue
        a, b = start[key], start[key + 1]
        if a == b: bucket[key] = None; continue
        s0, s1 = a // L, (b - 1) // L
        if s0 == s1: assert key in bucket; continue
        ln = Lane(cv); acc = None
        for s in range(s0, s1 + 1): acc = ln.add(acc, partial[2 * s + (0 if a <= s * L else 1)])
        assert key not in bucket; bucket[key] = acc
        stats["combine"] = max(stats.get("combine", 0), ln.ops)
    # 4. the bucket reduction in chunks of m, then the tree per window
    per_window = S["per_window"]
    window_sum = []
    for w in range(W):
        chunks = []
        for j in range(per_window):
            ln = Lane(cv); off = j * m; base = (w << c) + off
            run = tot = None
            for t in range(m - 1, -1, -1):
                if off + t: run = ln.add(run, bucket[base + t])
                if t: tot = ln.add(tot, run)
            mult = None
            for bit in range(c - 1, -1, -1):
                mult = ln.dbl(mult)
                if (off >> bit) & 1: mult = ln.add(mult, run)
            chunks.append(ln.add(tot, mult))
            stats["chunks"] = max(stats.get("chunks", 0), ln.ops)
        window_sum.append(tree_sum(cv, chunks, stats))
    # 5. the windows
    ln = Lane(cv); acc = None
    for w in range(W - 1, -1, -1):
        for _ in range(c): acc = ln.dbl(acc)
        acc = ln.add(acc, window_sum[w])
    stats["final"] = ln.ops
    return acc, invalid, stats


def point_sum(cv, pts):
    """ecsimd_msm_point_sum index by index: (the affine sum or None, invalid, stats)."""
    n, stats = len(pts), {}
    if n == 0: return None, 0, stats
    cls = [classify(cv, pt) for pt in pts]
    lanes = ceil_div(n, TREE_FAN)
    arr = []
    for g in range(lanes):
        ln = Lane(cv); acc = None
        for t in range(TREE_FAN):
            e = g + t * lanes
            if e >= n: break
            if cls[e] == 1: acc = ln.add(acc, pts[e])
        arr.append(acc)
        stats["front"] = max(stats.get("front", 0), ln.ops)
    return tree_sum(cv, arr, stats), sum(1 for v in cls if v == 2), stats


def msm_reference(cv, ks, pts, bits=256):
    """sum (k mod 2^bits) P by the group law alone, invalid points and (0, 0) skipped: what every route must give."""
    acc = None
    for k, pt in zip(ks, pts):
        if classify(cv, pt) == 1: acc = ec_add(cv, acc, ec_mul(cv, k & ((1 << bits) - 1), pt))
    return acc
