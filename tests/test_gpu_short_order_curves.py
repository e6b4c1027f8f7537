"""Curves registered with a group order n < 2^255: no comb, no per-lane window table, and -- since the reference's ladder, which alone could serve them, is
wrong wherever k | 1 = 2^j mod n for bitlen(n) <= j <= 256 (tools/ladder_degenerate_model.py, tests/test_ladder_degenerate_cpu.py) -- no ECDSA either.
Checked here on the device: the capabilities, the refusal of every entry point over that route, and that the device ladder on the generator is wrong at
exactly the scalars the model lists (affine, against textbook arithmetic on Python integers: exact, no tolerance) -- the reason for the refusal.

Predicted from the oracle, not measured on a device: before this change these ids had the ECDSA capability, and ecdsa_sign(P-192, nonce 2^192 - n) would
return r from the ladder's (0, 0).  The last test here measures the device ladder at those scalars, which is that route's only source of points.
"""
import json
import os
import sys

import numpy as np
import pytest

from helpers import SEED, to_int, ints_to_arr

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools"))
import ladder_degenerate_model as model     # noqa: E402
import short_order_curves as curves          # noqa: E402

pytestmark = pytest.mark.gpu
OUT_AFFINE = 2
TINY = curves.tiny_curves()
CURVES = {"p192": curves.P192, "tiny8_a-3": TINY["tiny8_a-3"], "tiny13_arandom": TINY["tiny13_arandom"]}      # registration needs p >= 7; both tiny p >= 2^7
with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "short_order_curves.json")) as f:
    CURVES.update({name: {k: int(v, 16) for k, v in c.items()} for name, c in json.load(f).items()})          # cm255, cm224 (tools/short_order_curves.py)


def register(c):
    from ecsimd_amd.engine import register_curve
    return register_curve(c["p"], c["a"], c["b"], c["gx"], c["gy"], c["n"])


@pytest.mark.parametrize("name", list(CURVES))
def test_capabilities_follow_the_registration_rule(engine, name):
    from ecsimd_amd.engine import curve_capabilities, CURVE_HAS_ORDER, CURVE_COMB, CURVE_ECDSA, CURVE_WINDOW_VARIABLE_BASE
    c = CURVES[name]
    assert curves.validate(c) and c["n"] < 2 ** 255
    caps = curve_capabilities(register(c))
    assert caps & CURVE_HAS_ORDER and not caps & CURVE_COMB and not caps & CURVE_WINDOW_VARIABLE_BASE
    assert not caps & CURVE_ECDSA                                                 # the rule: n >= 2^255, p < 2n, n G = O where n is a prime in p's Hasse interval


def test_the_other_side_of_the_rule_and_a_wrong_prime_order(engine):
    """brainpoolP256r1 with its order: every capability.  With the next prime above n (inside p's Hasse interval, passes Miller-Rabin, and is not the order
    of G): HAS_ORDER alone -- the comb, the window loop and ECDSA all compute modulo n -- and each is refused; the ladder still serves the id."""
    from ecsimd_amd import EcsimdHipError, ALG_WINDOWED
    from ecsimd_amd.engine import register_curve, curve_capabilities, CURVE_HAS_ORDER, CURVE_COMB, CURVE_ECDSA, CURVE_WINDOW_VARIABLE_BASE
    from oracle.loader import REF_CURVES
    c = REF_CURVES["brainpoolP256r1"]
    good = register_curve(c["p"], c["a"], c["b"], c["gx"], c["gy"], c["n"])
    assert curve_capabilities(good) == CURVE_HAS_ORDER | CURVE_COMB | CURVE_ECDSA | CURVE_WINDOW_VARIABLE_BASE
    near = c["n"] + 2
    while not curves.is_prime(near):
        near += 2
    assert (near - c["p"] - 1) ** 2 < 4 * c["p"] and near >> 255
    _, mul = curves.affine_model(c)
    assert mul(near, (c["gx"], c["gy"])) is not None
    wrong = register_curve(c["p"], c["a"], c["b"], c["gx"], c["gy"], near)
    assert wrong != good and curve_capabilities(wrong) == CURVE_HAS_ORDER
    k = engine.fill_random(8, SEED, 3)
    lx, ly = engine.scalar_mult_base(wrong, k, flags=OUT_AFFINE)
    gx_, gy_ = engine.scalar_mult_base(good, k, flags=OUT_AFFINE)
    assert np.array_equal(engine.to_numpy(lx), engine.to_numpy(gx_)) and np.array_equal(engine.to_numpy(ly), engine.to_numpy(gy_))
    for call in (lambda: engine.scalar_mult_base(wrong, k, flags=OUT_AFFINE | ALG_WINDOWED), lambda: engine.scalar_mult(wrong, k, lx, ly, flags=OUT_AFFINE | ALG_WINDOWED),
                 lambda: engine.ecdsa_sign(wrong, k, k, k), lambda: engine.ecdsa_verify(wrong, k, k, k, lx, ly)):
        with pytest.raises(EcsimdHipError, match=r"n >= 2\^255"):
            call()


@pytest.mark.parametrize("name", list(CURVES))
def test_every_entry_point_over_the_ladder_route_is_refused(engine, name):
    from ecsimd_amd import EcsimdHipError, ALG_WINDOWED, ALG_CONSTANT_TIME
    c = CURVES[name]
    cid = register(c)
    n_ = c["n"]
    rng = np.random.default_rng(sum(name.encode()))
    up = engine.to_device
    for m in (1, 3, 257):
        v = up(ints_to_arr([int.from_bytes(rng.bytes(32), "big") % (n_ - 1) + 1 for _ in range(m)]))
        qx, qy = engine.scalar_mult_base(cid, v, flags=OUT_AFFINE)
        rid = engine.flags(m)                                                     # (refused before anything is read)
        calls = [lambda: engine.ecdsa_sign(cid, v, v, v), lambda: engine.ecdsa_sign_recoverable(cid, v, v, v), lambda: engine.ecdsa_sign_recoverable(cid, v, v, v, low_s=True),
                 lambda: engine.ecdsa_verify(cid, v, v, v, qx, qy), lambda: engine.double_scalar_mult(cid, v, v, qx, qy), lambda: engine.ecdsa_verify_rx(cid, v, v, qx, qy, v), lambda: engine.ecdsa_recover(cid, v, v, v, rid)]
        for call in calls:
            with pytest.raises(EcsimdHipError, match=r"n >= 2\^255"):
                call()
        for call in (lambda: engine.rfc6979_nonce(cid, v, v), lambda: engine.ecdsa_sign_deterministic(cid, v, v)):
            with pytest.raises(EcsimdHipError, match="qlen = 256"):
                call()
        for fl in (OUT_AFFINE | ALG_WINDOWED, OUT_AFFINE | ALG_WINDOWED | ALG_CONSTANT_TIME):
            with pytest.raises(EcsimdHipError, match=r"n >= 2\^255"):
                engine.scalar_mult_base(cid, v, flags=fl)
            with pytest.raises(EcsimdHipError, match=r"n >= 2\^255"):
                engine.scalar_mult(cid, v, qx, qy, flags=fl)


@pytest.mark.parametrize("name", list(CURVES))
def test_the_device_ladder_is_wrong_exactly_where_the_model_says(engine, name):
    """scalar_mult_base(OUT_AFFINE) on these ids is the ladder.  Against textbook affine arithmetic: wrong at every scalar of degenerate_scalars(n) but 0, right at
    their neighbours that are not listed, at the images n - k that are not listed, and at seeded random scalars, up to 256 lanes and on ragged sizes."""
    c = CURVES[name]
    cid = register(c)
    n_, G = c["n"], (c["gx"], c["gy"])
    _, mul = curves.affine_model(c)
    dg = model.degenerate_scalars(n_)
    rng = np.random.default_rng(sum(name.encode()) + 1)
    pick = dg if len(dg) <= 40 else dg[:20] + dg[-20:]
    ks = list(dict.fromkeys(pick + [k + d for k in pick for d in (-1, 1) if 0 <= k + d < n_] + [n_ - k for k in pick if k]))[:200]
    ks += [int.from_bytes(rng.bytes(32), "big") % n_ for _ in range(256 - len(ks))]
    assert name != "p192" or (2 ** 192 - n_ in ks and 2 ** 192 - n_ - 1 in ks)
    for m in (len(ks), 1, 3):
        ax, ay = (engine.to_numpy(t) for t in engine.scalar_mult_base(cid, engine.to_device(ints_to_arr(ks[:m])), flags=OUT_AFFINE))
        wrong = [k for i, k in enumerate(ks[:m]) if (to_int(ax[i]), to_int(ay[i])) != (mul(k, G) or (0, 0))]
        assert sorted(set(wrong)) == sorted(k for k in set(ks[:m]) if k and k in set(dg)), (name, m, [hex(k) for k in wrong][:8])
