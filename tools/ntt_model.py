#!/usr/bin/env python3
"""The number-theoretic transform of include/ecsimd_ntt.h, defined with plain Python integers.

What the library computes, stated independently of it:
  * two_adicity(p), default_root(p): s with 2^s || p - 1, and g^((p - 1) / 2^s) for the smallest integer g >= 2 that is a quadratic non-residue;
  * the BLS12-381 scalar field Fr and its conventional root 7^((r - 1) / 2^32) (checked at import: order exactly 2^32; 5, not 7, is the smallest non-residue);
  * dft(): the O(n^2) definition  out[k] = sum_i in[i] (g w^k)^i;  ntt(): a recursive transform held to it for n <= 64 (self_check);
  * forward() / inverse() on a subgroup or a coset, bitrev(), poly_mul();
  * plan(): the schedule ecsimd_ntt_plan reports, restated;  passes(): the transform pass by pass with the index formulas of ecsimd_amd/csrc/ntt.cuh, restated
    (columns, bit-reversed rows, decimation-in-time stages, the twiddle between passes, the two-level tables, the buffer each pass writes).

`python tools/ntt_model.py` rewrites tests/golden/ntt_vectors.json; tests/test_ntt_cpu.py holds the file to this module byte for byte."""
import json
import os
import random

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VECTORS_PATH = os.path.join(ROOT, "tests", "golden", "ntt_vectors.json")

# ---- fields
FR = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001          # the order of BLS12-381's G1, G2, GT
FR_ROOT = 0x16a2a19edfe81f20d09b681922c813b4b63683508c2280b93829971f439f0d2b     # 7^((r - 1) / 2^32)
P256_ORDER = 0xffffffff00000000ffffffffffffffffbce6faada7179e84f3b9cac2fc632551


def two_adicity(p):
    s, m = 0, p - 1
    while m % 2 == 0:
        s, m = s + 1, m // 2
    return s


def is_residue(g, p):
    return pow(g, (p - 1) // 2, p) == 1


def smallest_non_residue(p):
    g = 2
    while is_residue(g, p):
        g += 1
    return g


def default_root(p):
    """the 2^s-th primitive root ecsimd_ntt_field_info returns"""
    return pow(smallest_non_residue(p), (p - 1) >> two_adicity(p), p)


def is_root_of_order(root, s, p):
    """root has order exactly 2^s"""
    return 0 < root < p and pow(root, 1 << (s - 1), p) == p - 1


def is_prime(n):
    """Miller-Rabin with the first 24 primes as bases: deterministic here, and far more than the primes this file meets need"""
    small = (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37, 41, 43, 47, 53, 59, 61, 67, 71, 73, 79, 83, 89)
    if n < 2:
        return False
    for q in small:
        if n % q == 0:
            return n == q
    d, s = n - 1, 0
    while d % 2 == 0:
        d, s = d // 2, s + 1
    for a in small:
        x = pow(a, d, n)
        if x in (1, n - 1):
            continue
        for _ in range(s - 1):
            x = x * x % n
            if x == n - 1:
                break
        else:
            return False
    return True


def dense_prime():
    """the largest prime 2^256 - 2^8 j + 1: its top word is all ones (Fr's is 0x73eda753) and its two-adicity at least 8"""
    j = 1
    while not is_prime((1 << 256) - (j << 8) + 1):
        j += 1
    return (1 << 256) - (j << 8) + 1


assert two_adicity(FR) == 32 and is_prime(FR)
assert FR_ROOT == pow(7, (FR - 1) >> 32, FR) and is_root_of_order(FR_ROOT, 32, FR)
assert smallest_non_residue(FR) == 5 and not is_residue(7, FR) and default_root(FR) != FR_ROOT


# ---- the transform
def domain_omega(p, log_n, root=None):
    s = two_adicity(p)
    root = default_root(p) if root is None else root
    if not 1 <= log_n <= min(s, MAX_LOG_N) or not is_root_of_order(root, s, p):
        raise ValueError("log_n or root")
    return pow(root, 1 << (s - log_n), p)


def dft(x, w, p, g=1):
    """the definition: out[k] = sum_i x[i] (g w^k)^i"""
    n = len(x)
    return [sum(x[i] * pow(g * pow(w, k, p), i, p) for i in range(n)) % p for k in range(n)]


def ntt(x, w, p):
    """out[k] = sum_i x[i] w^(i k), recursively (decimation in time); w of order len(x)"""
    n = len(x)
    if n == 1:
        return [x[0] % p]
    even, odd = ntt(x[0::2], w * w % p, p), ntt(x[1::2], w * w % p, p)
    out, t = [0] * n, 1
    for k in range(n // 2):
        out[k], out[k + n // 2] = (even[k] + t * odd[k]) % p, (even[k] - t * odd[k]) % p
        t = t * w % p
    return out


def forward(x, p, log_n, root=None, shift=1):
    w, n = domain_omega(p, log_n, root), 1 << log_n
    assert len(x) == n and 0 < shift < p
    scaled, t = [], 1
    for v in x:
        scaled.append(v * t % p)
        t = t * shift % p
    return ntt(scaled, w, p)


def inverse(y, p, log_n, root=None, shift=1):
    w, n = domain_omega(p, log_n, root), 1 << log_n
    assert len(y) == n and 0 < shift < p
    x = ntt(y, pow(w, p - 2, p), p)
    ninv, ginv, t, out = pow(n, p - 2, p), pow(shift, p - 2, p), 1, []
    for v in x:
        out.append(v * ninv % p * t % p)
        t = t * ginv % p
    return out


def bitrev_index(i, bits):
    r = 0
    for b in range(bits):
        r |= ((i >> b) & 1) << (bits - 1 - b)
    return r


def bitrev(x, log_n):
    out = [0] * len(x)
    for i, v in enumerate(x):
        out[bitrev_index(i, log_n)] = v
    return out


def poly_mul(a, b, p, log_n, root=None):
    fa, fb = forward(a, p, log_n, root), forward(b, p, log_n, root)
    return inverse([u * v % p for u, v in zip(fa, fb)], p, log_n, root)


def horner(x, z, p):
    acc = 0
    for v in reversed(x):
        acc = (acc * z + v) % p
    return acc


# ---- the schedule (ecsimd_amd/csrc/ntt.cuh make_schedule, ecsimd_ntt_plan)
TILE_LOG, LANES, DEFAULT_RADIX_LOG, MAX_LOG_N, MAX_PASSES, SPLIT_LOG = 11, 256, 9, 24, 24, 12
LDS_BYTES = 2 * ((1 << TILE_LOG) + (1 << DEFAULT_RADIX_LOG)) * 16


def max_radix_log(r):
    """ECSIMD_NTT_MAX_RADIX_LOG(r)"""
    return r & 15


def plan(log_n, batch=1, flags=0):
    cap = flags & 15 or DEFAULT_RADIX_LOG
    if flags & ~15 or not 1 <= cap <= DEFAULT_RADIX_LOG or not 1 <= log_n <= MAX_LOG_N or not 1 <= batch <= (1 << 38) >> log_n:
        raise ValueError("log_n, batch or flags")
    passes = -(-log_n // cap)
    base, rem = divmod(log_n, passes)
    radix = [base + (1 if i < rem else 0) for i in range(passes)]
    return {"passes": passes, "log_radix": radix + [0] * (MAX_PASSES - passes), "lanes": LANES, "lds_bytes": LDS_BYTES, "launches": passes,
            "workspace_bytes": (batch << log_n) * 32 if passes > 1 else 0}


def passes(x, p, log_n, root=None, shift=1, inverse_=False, flags=0, trace=None):
    """forward() or inverse() of ONE array the way the device does it: pass by pass, column by column.  trace (a list) receives, per pass, the buffer it wrote
    ('workspace' or 'out') and the array after it."""
    n, pl = 1 << log_n, plan(log_n, 1, flags)
    w = domain_omega(p, log_n, root)
    if inverse_:
        w, g = pow(w, p - 2, p), pow(shift, p - 2, p)
    else:
        g = shift
    split = 1 << SPLIT_LOG
    lo = [pow(w, i, p) for i in range(min(n, split))]
    hi = [pow(w, split * i, p) for i in range(max(1, n >> SPLIT_LOG))]
    glo = [pow(g, i, p) for i in range(min(n, split))]
    ghi = [pow(g, split * i, p) for i in range(max(1, n >> SPLIT_LOG))]
    log_rt = min(log_n, DEFAULT_RADIX_LOG)
    stage_table = [pow(w, i << (log_n - log_rt), p) for i in range(1 << (log_rt - 1))]
    cur, log_s = [v % p for v in x], 0
    for i in range(pl["passes"]):
        log_r = pl["log_radix"][i]
        r, log_w = 1 << log_r, log_n - log_r
        first, last = i == 0, i + 1 == pl["passes"]
        nxt = [None] * n
        for c in range(1 << log_w):
            rows = [None] * r
            for j in range(r):
                idx = c + (j << log_w)
                v = cur[idx]
                if first and not inverse_:
                    v = v * (glo[idx & (split - 1)] * ghi[idx >> SPLIT_LOG] % p) % p
                rows[bitrev_index(j, log_r)] = v
            for u in range(log_r):
                for h in range(r // 2):
                    low = h & ((1 << u) - 1)
                    j0 = ((h >> u) << (u + 1)) | low
                    a, b = rows[j0], rows[j0 + (1 << u)] * stage_table[low << (log_rt - 1 - u)] % p
                    rows[j0], rows[j0 + (1 << u)] = (a + b) % p, (a - b) % p
            q, pp = c & ((1 << log_s) - 1), c >> log_s
            for k in range(r):
                dst = q + (k << log_s) + (pp << (log_s + log_r))
                v = rows[k]
                if not last:
                    e = (pp * k) << log_s
                    assert e < n
                    v = v * (lo[e & (split - 1)] * hi[e >> SPLIT_LOG] % p) % p
                elif inverse_:
                    v = v * pow(n, p - 2, p) % p * (glo[dst & (split - 1)] * ghi[dst >> SPLIT_LOG] % p) % p
                assert nxt[dst] is None
                nxt[dst] = v
        cur, log_s = nxt, log_s + log_r
        if trace is not None:
            trace.append(("workspace" if (not last and i % 2 == 0) else "out", list(cur)))
    return cur


def self_check():
    rng = random.Random(0x6e7474)
    for p in (FR, P256_ORDER, dense_prime()):
        s = two_adicity(p)
        assert is_root_of_order(default_root(p), s, p)
        for log_n in range(1, min(s, 6) + 1):
            n = 1 << log_n
            w = domain_omega(p, log_n)
            x = [rng.randrange(p) for _ in range(n)]
            for shift in (1, 7, rng.randrange(1, p)):
                want = dft(x, w, p, shift)
                assert forward(x, p, log_n, None, shift) == want
                assert inverse(want, p, log_n, None, shift) == x
                for cap in (0, 1, 2, 3):
                    assert passes(x, p, log_n, None, shift, False, cap) == want, (log_n, cap)
                    assert passes(want, p, log_n, None, shift, True, cap) == x, (log_n, cap)
    for log_n in (10, 11):                                                              # the default schedule's two-pass sizes, against the recursive transform
        x = [rng.randrange(FR) for _ in range(1 << log_n)]
        assert passes(x, FR, log_n, FR_ROOT) == forward(x, FR, log_n, FR_ROOT)
    a, b = [rng.randrange(FR) for _ in range(8)], [rng.randrange(FR) for _ in range(8)]
    school = [0] * 16
    for i, u in enumerate(a):
        for j, v in enumerate(b):
            school[i + j] = (school[i + j] + u * v) % FR
    assert poly_mul(a + [0] * 8, b + [0] * 8, FR, 4, FR_ROOT) == school
    assert bitrev(list(range(8)), 3) == [0, 4, 2, 6, 1, 5, 3, 7]
    return True


# ---- the cases of tests/cpp/ntt_host_check.cpp (its header has the format)
def edge_inputs(p, n, rng):
    """the inputs every comparison uses: random values, 0 / 1 / p - 1, values from p up to 2^256 - 1"""
    x = [rng.randrange(p) for _ in range(n)]
    for i, v in zip(rng.sample(range(n), min(n, 6)), (0, 1, p - 1, p, (1 << 256) - 1, rng.randrange(p, 1 << 256))):
        x[i] = v
    return x


def host_check_cases(p=FR, root=FR_ROOT, log_ns=range(1, 13)):
    rng = random.Random(0x686f7374)
    lines = ["field %x %x %d" % (p, root, two_adicity(p))]
    for log_n in log_ns:
        todo = [(1, 1)] + ([(7, 1), (rng.randrange(2, p), 1)] if log_n in (1, 5, 12) else []) + ([(1, 3), (7, 67)] if log_n in (1, 3, 6) else [])
        for shift, batch in todo:
            xs = [edge_inputs(p, 1 << log_n, rng) for _ in range(batch)]
            lines.append("case %d %x %d" % (log_n, shift, batch))
            lines += ["%x" % v for x in xs for v in x]
            lines += ["%x" % v for x in xs for v in forward(x, p, log_n, root, shift)]
    return "\n".join(lines) + "\n"


# ---- the fixture
def vectors():
    rng = random.Random(0x4e5454)
    out = {"fr": {"modulus": hex(FR), "two_adicity": two_adicity(FR), "root": hex(FR_ROOT), "root_generator": 7, "smallest_non_residue": smallest_non_residue(FR),
                  "default_root": hex(default_root(FR))},
           "p256_order": {"modulus": hex(P256_ORDER), "two_adicity": two_adicity(P256_ORDER), "default_root": hex(default_root(P256_ORDER))},
           "dense_prime": {"modulus": hex(dense_prime()), "two_adicity": two_adicity(dense_prime()), "default_root": hex(default_root(dense_prime()))},
           "transforms": [], "plans": {}}
    for log_n in (3, 4):
        x = [rng.randrange(FR) for _ in range(1 << log_n)]
        x[1] = (1 << 256) - 1                                                           # an input above the modulus
        for shift in (1, 7):
            y = forward(x, FR, log_n, FR_ROOT, shift)
            out["transforms"].append({"log_n": log_n, "shift": shift, "in": [hex(v) for v in x], "forward": [hex(v) for v in y],
                                      "inverse": [hex(v) for v in inverse(x, FR, log_n, FR_ROOT, shift)]})
    for cap in (0, 2, 3):
        out["plans"][str(cap)] = [{k: v for k, v in plan(log_n, 1, cap).items() if k != "log_radix"} | {"log_radix": plan(log_n, 1, cap)["log_radix"][:plan(log_n, 1, cap)["passes"]]}
                                  for log_n in range(1, MAX_LOG_N + 1)]
    return out


def vectors_text():
    return json.dumps(vectors(), indent=1, sort_keys=True) + "\n"


if __name__ == "__main__":
    self_check()
    with open(VECTORS_PATH, "w") as f:
        f.write(vectors_text())
    print("wrote", VECTORS_PATH, len(vectors_text()), "bytes")
