"""Where the reference's co-Z Joye ladder returns a wrong point, for a generator of any prime order n: tools/ladder_degenerate_model.py against three witnesses --
the C oracle (the restatement the GPU ladder is held to bit for bit), textbook affine arithmetic on Python integers, and the tabulated multiples of G.

Measured here (all six tiny curves, every k in [0, 2n)): the shadow's flags minus the oracle's wrong scalars are exactly the k = 0 mod n -- two per curve, k = 0
("final_sub_infinity", or "zdau_sum_infinity" where some 2^j = 1 mod n) and k = n ("zdau_sum_infinity") -- where the ladder's (0, 0) IS the point at infinity.  Nothing else is over-predicted, so the test
asserts that equality.

Not covered: secp192k1 (its generator and order could not be reproduced from memory, and nothing can be looked up).  An order below 2^255 under a 256-bit p
with its top bit set and p < 2n does not exist among the j = 0 curves (it needs cofactor 2; their even orders are multiples of 4: tools/short_order_curves.py),
and an order of 224 bits under such a p breaks p < 2n: the fixtures cm255 and cm224 have p of the order's own size instead.
"""
import json
import os
import random
import sys

import numpy as np
import pytest

from oracle.loader import REF_CURVES, ints_to_arr, to_int, from_int
from helpers import CURVE_PARAMS, P256, SECP256K1

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools"))
import ladder_degenerate_model as model     # noqa: E402
import short_order_curves as curves          # noqa: E402

THREADS = min(16, os.cpu_count() or 1)
TINY = curves.tiny_curves()


def oracle_ladder_affine(oracle, c, ks):
    """(x, y) of the oracle's ladder on G followed by to_affine, per scalar; (0, 0) where Z = 0."""
    oid = oracle.register_curve(c["p"], c["a"], c["b"], c["gx"], c["gy"])
    m = len(ks)
    gx, gy = np.tile(from_int(c["gx"]), (m, 1)), np.tile(from_int(c["gy"]), (m, 1))
    ax, ay = oracle.to_affine(oid, oracle.scalar_mult(oid, ints_to_arr(ks), gx, gy, threads=THREADS))
    return [(to_int(x), to_int(y)) for x, y in zip(ax, ay)]


def test_the_generated_curves_span_the_sizes_and_shapes():
    assert len(TINY) >= 6 and min(c["p"] for c in TINY.values()) < 2 ** 7 and max(c["p"] for c in TINY.values()) > 2 ** 12
    assert {("0" if c["a"] == 0 else "-3" if c["a"] == c["p"] - 3 else "random") for c in TINY.values()} == {"0", "-3", "random"}
    for c in TINY.values():
        assert curves.validate(c) and c["p"] >= 7
        assert curves.count_points(c["p"], c["a"], c["b"]) == c["n"]
    assert TINY == curves.tiny_curves()                                            # the same curves from the same seeds, every time


@pytest.mark.parametrize("n", list(range(5, 400, 2)) + [65521, 65537])
def test_the_enumerator_is_the_shadow_below_n(n):
    """degenerate_scalars(n) is complete and exact: the set the shadow flags in [0, n), for every odd n (a group order or not: both are integer arithmetic)."""
    ks = range(n) if n < 1000 else set(model.degenerate_scalars(n)) | {k + d for k in model.degenerate_scalars(n) for d in (-1, 1) if 0 <= k + d < n} | set(random.Random(n).sample(range(n), 500))
    assert sorted(k for k in ks if model.shadow(k, n)) == model.degenerate_scalars(n)


@pytest.mark.parametrize("name", list(TINY))
def test_exhaustive_on_a_tiny_curve(oracle, name):
    c = TINY[name]
    n, G = c["n"], (c["gx"], c["gy"])
    add, mul = curves.affine_model(c)
    table, R = [], None                                                            # all multiples of G
    for _ in range(n):
        table.append(R if R is not None else (0, 0)); R = add(R, G)
    assert R is None and len(set(table)) == n
    ks = list(range(2 * n))
    assert all((mul(k, G) or (0, 0)) == table[k % n] for k in ks[::7])             # the two Python witnesses agree
    got = oracle_ladder_affine(oracle, c, ks)
    observed = {k for k in ks if got[k] != table[k % n]}
    why = {k: model.shadow(k, n) for k in ks}
    predicted = {k for k in ks if why[k]}
    assert observed <= predicted, sorted(observed - predicted)[:8]                 # sound: the condition that is never relaxed
    assert sorted(k for k in predicted if k < n) == model.degenerate_scalars(n)   # the enumerator is complete
    over = predicted - observed
    reasons = {}
    for k in over:
        reasons[why[k]] = reasons.get(why[k], 0) + 1
    print(name, "n =", n, "observed", len(observed), "predicted", len(predicted), "over-predicted", sorted(over), reasons)
    assert all(why[k] in model.INFINITY_REASONS for k in over)
    assert over == {0, n}                                                          # exactly the scalars whose product is the point at infinity
    # the images n - k: whether ECDSA's substitution could work here
    bad = set(model.degenerate_scalars(n))
    assert model.substitution_is_sound(n) == (not any((n - k) in observed for k in bad if k))


def test_p192(oracle):
    c = curves.P192
    n = c["n"]
    assert curves.validate(c)
    _, mul = curves.affine_model(c)
    dg = model.degenerate_scalars(n)
    assert {2 ** 192 - n, 2 ** 192 - n - 1} <= set(dg) and dg == sorted({0, n - 1, 2 ** 192 - n, 2 ** 192 - n - 1})
    rng = random.Random(192)
    images = [n - k for k in dg if k]
    ks = sorted(set(dg) | {k + d for k in dg for d in (-1, 1) if 0 <= k + d < n} | set(images) | {rng.randrange(n) for _ in range(200)})
    got = oracle_ladder_affine(oracle, c, ks)
    wrong = [k for k, g in zip(ks, got) if g != (mul(k, (c["gx"], c["gy"])) or (0, 0))]
    assert wrong == [k for k in dg if k], [hex(k) for k in wrong]                   # (k = 0: flagged, and (0, 0) is right)
    assert not set(images) & set(wrong) and model.substitution_is_sound(n)


@pytest.mark.parametrize("name", list(REF_CURVES) + ["p256", "secp256k1"])
def test_orders_of_256_bits_have_the_known_three(name):
    n = REF_CURVES[name]["n"] if name in REF_CURVES else CURVE_PARAMS[P256 if name == "p256" else SECP256K1]["n"]
    assert n >> 255
    assert model.degenerate_scalars(n) == sorted({0} | {k for k in (n - 1, 2 ** 256 - n - 1, 2 ** 256 - n) if 0 <= k < n})    # (0: flagged, and its (0, 0) is right)
    assert model.substitution_is_sound(n)
    rng = random.Random(name)
    for k in model.degenerate_scalars(n) + [n - k for k in model.degenerate_scalars(n) if k] + [rng.randrange(n) for _ in range(40)]:
        assert bool(model.shadow(k, n)) == (k in model.degenerate_scalars(n))


with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "short_order_curves.json")) as _f:
    CM = {name: {k: int(v, 16) for k, v in c.items()} for name, c in json.load(_f).items()}


@pytest.mark.parametrize("name", ["cm255", "cm224"])
def test_complex_multiplication_fixtures(oracle, name):
    """tests/golden/short_order_curves.json, re-validated in the Python model (on the curve, n prime, n G = O, p < 2n), then the oracle's ladder against
    textbook arithmetic: wrong at exactly degenerate_scalars(n) but 0 among that set, its neighbours, the images n - k and 200 seeded random scalars."""
    c = CM[name]
    n = c["n"]
    bits = {"cm255": 255, "cm224": 224}[name]
    assert curves.validate(c) and n.bit_length() == bits and c["p"].bit_length() == bits and c["a"] == 0
    _, mul = curves.affine_model(c)
    dg = model.degenerate_scalars(n)
    assert len(dg) > 4                                                              # more than the three (and 0): what the short order adds
    rng = random.Random(bits)
    images = [n - k for k in dg if k]
    ks = sorted(set(dg) | {k + d for k in dg for d in (-1, 1) if 0 <= k + d < n} | set(images) | {rng.randrange(n) for _ in range(200)})
    got = oracle_ladder_affine(oracle, c, ks)
    wrong = [k for k, g in zip(ks, got) if g != (mul(k, (c["gx"], c["gy"])) or (0, 0))]
    assert wrong == [k for k in dg if k], [hex(k) for k in wrong][:8]
    assert not set(images) & set(wrong) and model.substitution_is_sound(n)


def test_the_fixture_is_what_the_generator_prints():
    assert CM["cm224"] == curves.cm_curve(*curves.CM["cm224"])                      # (cm255 the same way: tools/short_order_curves.py; one search is enough per run)
