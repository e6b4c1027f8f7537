"""The CPU half of the schedule tests of the multi-scalar multiplication (tests/test_gpu_msm_schedule.py has the GPU half): the generators of tests/msm_cases.py
are held to the conditions the GPU test relies on, and to the schedule -- of tools/msm_model.py and of the library's ecsimd_msm_plan, which needs no GPU.

  widths    the parametrisation reaches every window width c = 1 .. 16 and tree depths 1, 2 and 3; the tabulated rows are what the planner gives.
  one-hot   every window -- so every window that straddles a 32-bit word -- meets every digit pattern, and every scalar has the one digit it says it has.
  layouts   per shape, the 64 batches reach all 17 classes of a bucket's position over the slices; each batch goes through the model's index-level emulation of
            the bucket route, with a shuffled order inside the buckets, against the big-int sum.
"""
import os
import random
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import msm_cases as cases                                       # noqa: E402
import msm_model as model                                       # noqa: E402
from helpers import CURVE_PARAMS, P256, SECP256K1, ec_mul       # noqa: E402

CSRC = os.path.join(ROOT, "ecsimd_amd", "csrc")
BUCKETS, LANES, AUTO = cases.BUCKETS, cases.LANES, cases.AUTO


@pytest.fixture(scope="module")
def built():
    import ecsimd_amd
    subprocess.run(["make", "-j", str(min(8, os.cpu_count() or 1)), "-C", CSRC, "ARCH=gfx950"], check=True, capture_output=True, timeout=1800)
    return ecsimd_amd.load_library()


def both_plans(n, bits, alg):
    from ecsimd_amd import Engine
    got, want = Engine.msm_plan(n, bits, alg), model.plan(n, bits, alg)
    assert got == want, (n, bits, alg, got, want)
    return got


# ---- 1. widths
def test_the_width_cases_reach_every_c_and_every_tree_depth(built):
    for c, n, windows, m, L, per_window, passes in cases.WIDTH_TABLE:
        plan = both_plans(n, 256, BUCKETS)
        assert (plan["c"], plan["windows"], plan["m"], plan["L"], plan["buckets"] // plan["m"], cases.tree_passes(plan)) == (c, windows, m, L, per_window, passes), (c, n)
        assert (c, n, 256) in cases.WIDTH_CASES
    seen_c, seen_depth = set(), set()
    for c, n, bits in cases.WIDTH_CASES:
        plan = both_plans(n, bits, BUCKETS)
        assert plan["c"] == c and plan["windows"] * c >= bits > (plan["windows"] - 1) * c, (c, n, bits)
        if c > 2: assert model.plan(n - 1, bits, BUCKETS)["c"] < c, (c, n)                                # the smallest n that gives this c
        assert plan["launches"] == 8 + cases.tree_passes(plan)
        seen_c.add(c); seen_depth.add(cases.tree_passes(plan))
    assert seen_c == set(range(1, 17)) and seen_depth == {0, 1, 2, 3}, (seen_c, seen_depth)             # a condition, not a hope (0: one chunk per window, c <= 2)
    assert both_plans((1 << 20) - 1, 256, AUTO)["route"] == LANES and both_plans(1 << 20, 256, AUTO)["route"] == BUCKETS
    assert max(n for _, n, _ in cases.WIDTH_CASES) == model.AUTO_THRESHOLD == cases.LANES_MAX_N
    for c, n, bits in cases.PARTIAL_TOP_CASES:
        plan = both_plans(n, bits, BUCKETS)
        assert plan["c"] == c and bits % c and c & (c - 1), (c, n, bits)                                  # a partial top window, no power of two
        assert cases.straddling_windows(c, plan["windows"]), (c, bits)
    assert {(c, n) for c, n, _ in cases.PARTIAL_TOP_CASES} == {(7, 2048), (9, 8192), (11, 32768), (13, 131072)}
    assert {bits for _, _, bits in cases.PARTIAL_TOP_CASES} == {255, 129}
    assert len(set(cases.WIDTH_CASES + cases.PARTIAL_TOP_CASES)) == 16 + 8


def test_width_batches_are_distinct_and_their_host_sum_is_exact():
    for c, n, bits in cases.WIDTH_CASES + cases.PARTIAL_TOP_CASES:
        for cv in cases.CURVES:
            a, k = cases.width_batch(cv, n, bits)
            assert a.shape == (n,) and k.shape == (n, 4) and a.dtype == k.dtype == np.uint64
            assert a.min() >= 1 and a.max() < 1 << 63 and len(np.unique(a)) == n                        # distinct points
            assert len(np.unique(k[:, 0])) == n                                                           # distinct scalars (already in the low limb)
            if bits < 256: assert (k != cases.mask_limbs(k, bits)).any()                                  # bits above `bits` are set: the device has to drop them
    for bits in (256, 255, 129, 64, 1):
        for cv in cases.CURVES:
            order = CURVE_PARAMS[cv]["n"]
            a, k = cases.width_batch(cv, 300, bits)
            ks = cases.ints_of(k)
            assert cases.limbs_of(ks).tolist() == k.tolist()
            assert cases.dot_mod(k, a, bits, order) == sum((kv % (1 << bits)) * int(av) for kv, av in zip(ks, a)) % order


def test_the_chunk_sum_by_residues_is_the_plain_sum(built):
    k = np.random.default_rng(5).integers(0, 1 << 64, size=(3 * cases.WALK + 17, 4), dtype=np.uint64, endpoint=False)
    order = CURVE_PARAMS[P256]["n"]
    assert cases.chunk_dot(k, order) == sum(int(v) * (i % cases.WALK + 1) for i, v in enumerate(k[:, 0])) % order
    plan = both_plans(cases.CHUNK_N, cases.CHUNK_BITS, LANES)
    assert plan["launches"] == 4 + 5 * 2 + model.tree_passes(-(-cases.CHUNK_N // 16))                  # two chunks of the per-lane product
    assert model.VARWIN_CHUNK < cases.CHUNK_N < 2 * model.VARWIN_CHUNK and cases.CHUNK_N % cases.WALK


# ---- 2. one-hot windows
@pytest.mark.parametrize("bits", cases.ONE_HOT_BITS)
@pytest.mark.parametrize("c", cases.ONE_HOT_WIDTHS)
def test_one_hot_batches_put_every_pattern_into_every_straddling_window(c, bits):
    n = 1 << (c + 4)
    plan = model.plan(n, bits, BUCKETS)
    W = plan["windows"]
    assert plan["c"] == c and (c == 3 or model.plan(n - 1, bits, BUCKETS)["c"] < c)
    straddling = cases.straddling_windows(c, W)
    assert straddling == [w for w in range(W) if (w * c) // 32 != (w * c + c - 1) // 32]              # the first and the last bit lie in different words
    assert len([w for w in straddling if w * c + c <= bits]) >= 4
    met, values = set(), {}
    for ks, tags in cases.one_hot_batches(c, n, bits):
        assert len(ks) == len(tags) == n
        for i, (k, (w, name, d)) in enumerate(zip(ks, tags)):
            assert w == i % W and 0 < d < 1 << c and k < 1 << 256
            assert k == (d << (w * c)) % (1 << 256)                                                       # one digit, in window w, and nothing else
            digits = [(k >> (v * c)) & ((1 << c) - 1) for v in range(W)]
            assert all(dv == 0 for v, dv in enumerate(digits) if v != w)
            met.add((w, name)); values.setdefault(name, set()).add(d)
    assert values["one"] == {1} and values["all ones"] == {(1 << c) - 1} and values["top bit"] == {1 << (c - 1)} and values["below the top bit"] == {(1 << (c - 1)) - 1}
    assert values["alternating"] == {int(("10" * c)[:c], 2)} and (c == 3 or len(values["random"]) > 4)
    assert met == {(w, name) for w in range(W) for name in cases.PATTERNS}                              # every window, the straddling ones among them
    assert {(w, name) for w in straddling for name in cases.PATTERNS} <= met


def test_the_top_window_is_partial_and_differs_between_the_two_values_of_bits():
    for c in cases.ONE_HOT_WIDTHS:
        n = 1 << (c + 4)
        top = {bits: bits - c * (model.plan(n, bits, BUCKETS)["windows"] - 1) for bits in cases.ONE_HOT_BITS}
        assert all(1 <= v <= c for v in top.values()) and top[256] != top[255] and min(top.values()) < c, (c, top)
    assert {c for c in (3, 5) if 255 % c == 0} == {3, 5}                                                 # c = 3, 5: partial at 256, full at 255


def test_a_one_hot_batch_through_the_models_bucket_route():
    c, n = 3, 128
    for bits in cases.ONE_HOT_BITS:
        for cv in cases.CURVES:
            ks, _ = cases.one_hot_batches(c, n, bits)[cv]
            order = CURVE_PARAMS[cv]["n"]
            pts = cases.walk(cv)[:n]
            got, bad, _ = model.msm_buckets(cv, ks, pts, bits)
            assert bad == 0 and got == ec_mul(cv, sum((k % (1 << bits)) * (i + 1) for i, k in enumerate(ks)) % order, cases.G(cv))


# ---- 3. layouts
def test_the_classifier_tells_17_classes_apart():
    assert len(cases.all_layout_classes()) == cases.LAYOUT_CLASSES == 17
    L = 4
    assert cases.layout_class(5, 5, L) == "empty"
    assert cases.layout_class(4, 8, L) == (False, True, True, 0) and cases.layout_class(5, 7, L) == (False, False, False, 0)
    assert cases.layout_class(4, 7, L) == (False, True, False, 0) and cases.layout_class(5, 8, L) == (False, False, True, 0)
    assert cases.layout_class(4, 12, L) == (True, True, True, 0) and cases.layout_class(4, 16, L) == (True, True, True, 1) and cases.layout_class(4, 20, L) == (True, True, True, 2)
    assert cases.layout_class(3, 5, L) == (True, False, False, 0) and cases.layout_class(3, 9, L) == (True, False, False, 1) and cases.layout_class(3, 41, L) == (True, False, False, 2)
    assert cases.layout_class(3, 8, L) == (True, False, True, 0) and cases.layout_class(4, 9, L) == (True, True, False, 0)
    seen = {cases.layout_class(a, b, L) for a in range(0, 12) for b in range(a, 40)}
    assert seen == cases.all_layout_classes()


@pytest.mark.parametrize("n,bits", cases.LAYOUT_SHAPES)
def test_the_layout_batches_reach_all_17_classes_and_pass_the_models_bucket_route(built, n, bits):
    plan = both_plans(n, bits, BUCKETS)
    assert (plan["c"], plan["windows"], plan["L"]) == {(256, 4): (4, 1, 4), (257, 8): (4, 2, 8), (4099, 8): (8, 1, 32)}[(n, bits)]
    c, W, L = plan["c"], plan["windows"], plan["L"]
    if W == 2: assert n % L and (n // L) * L < n < (n // L + 1) * L                                       # the second window begins inside a slice
    reached, first_at = set(), {}
    shuffle_rng = random.Random(n)
    for index in range(cases.LAYOUT_BATCHES):
        ks, counts = cases.layout_batch(n, bits, index)
        assert len(ks) == n and len(counts) == W and all(len(cnt) == 1 << c and sum(cnt) == n for cnt in counts)
        for w, cnt in enumerate(counts):                                                                  # the scalars ARE the digits with these counts
            assert np.bincount([(k >> (w * c)) & ((1 << c) - 1) for k in ks], minlength=1 << c).tolist() == cnt
        assert max(ks) < 1 << bits
        for cls in cases.layout_classes_of(n, bits, counts):
            if cls not in reached: first_at[cls] = index
            reached.add(cls)
        cv = cases.CURVES[index % 2]
        order = CURVE_PARAMS[cv]["n"]
        got, bad, _ = model.msm_buckets(cv, ks, cases.walk(cv)[:n], bits, lambda idx: shuffle_rng.sample(idx, len(idx)))
        assert bad == 0 and got == ec_mul(cv, sum(k * (i + 1) for i, k in enumerate(ks)) % order, cases.G(cv)), index
    missing = cases.all_layout_classes() - reached
    assert not missing, (n, bits, missing)
    print(f"n = {n}, bits = {bits}, L = {L}: all 17 classes within {max(first_at.values()) + 1} batches")


# ---- 5. the operands
def test_b_is_a_square_on_p256_and_none_on_secp256k1():
    p = CURVE_PARAMS[P256]["p"]
    y = cases.sqrt_b(P256)
    assert y is not None and 0 < y < p and y * y % p == CURVE_PARAMS[P256]["b"]                          # (0, +-y) are points of P-256
    p = CURVE_PARAMS[SECP256K1]["p"]
    assert cases.sqrt_b(SECP256K1) is None and pow(7, (p - 1) // 2, p) == p - 1                           # Euler: 7 is no square, no point has x = 0
    for cv in cases.CURVES:
        order = CURVE_PARAMS[cv]["n"]
        ks = cases.order_edge_scalars(cv)
        assert len(set(ks)) == 5 and all(0 < k < 1 << 256 for k in ks) and [k % order for k in ks[:3]] == [order - 1, 0, 1]
