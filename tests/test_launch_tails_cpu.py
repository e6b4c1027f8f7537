"""The CPU half of the launch-level tests (tests/test_gpu_launch_tails.py has the GPU half and says what the whole is for).

Here: the order-parameterised models of tools/launch_tails_model.py agree, at the real order, with the models the suite already trusts and with the published
vectors; gmod_constants agrees with the library's and the oracle's constants of the two built-in orders and satisfies its defining congruences for a
surrogate one; every batch the GPU test runs has the lanes on both sides of the order that the GPU test says it has; and the probe compiles and links --
which also fails loudly if the launchers ever stop being exported.
"""
import ctypes as C
import hashlib
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bip32_model  # noqa: E402
import bip340_model  # noqa: E402
import btc_model  # noqa: E402
import ecdsa_recover_model  # noqa: E402
import launch_probe  # noqa: E402
import launch_tails_cases as cases  # noqa: E402
import launch_tails_model as model  # noqa: E402
import rfc6979_model  # noqa: E402

N, P = model.N, model.P
GOLDEN = os.path.join(ROOT, "tests", "golden")
SECP = dict(p=P, a=0, b=7, gx=model.GX, gy=model.GY, n=N)


def golden(name):
    with open(os.path.join(GOLDEN, name)) as f:
        return json.load(f)


def test_the_probe_compiles_and_links():
    """Linked afresh every time (file times do not decide it), with undefined symbols an error: a launcher that is no longer exported fails here."""
    import ecsimd_amd
    exported = subprocess.run(["nm", "-DC", "--defined-only", ecsimd_amd.lib_path()], capture_output=True, text=True, check=True).stdout
    for name in launch_probe.WRAPPERS:
        assert f" T ecsimd_hip::launch::{name}(" in exported, f"libecsimd_hip.so does not export launch::{name}"
    out = launch_probe.build_probe(force=True)
    assert os.path.exists(out) and os.path.getmtime(out) >= os.path.getmtime(ecsimd_amd.lib_path())
    syms = subprocess.run(["nm", "-D", out], capture_output=True, text=True, check=True).stdout
    for name in launch_probe.WRAPPERS:
        assert f" T probe_{name}\n" in syms, name
        assert any(line.startswith("                 U ") and f"launch{len(name)}{name}E" in line for line in syms.splitlines()), name      # resolved from the library at load time
    assert "__hip_fatbin" not in syms and "__hipRegisterFunction" not in syms      # no device code of its own


# ---- the models at the real order against the models the suite has
def test_constants_are_secp256k1s():
    assert (model.P, model.N, model.GX, model.GY) == (bip340_model.P, bip340_model.N, bip340_model.GX, bip340_model.GY)
    model.check_order(N); model.check_order(cases.HALF)


def test_bip32_models_agree_at_the_real_order():
    rng = random.Random(1)
    for length in (16, 33, 64):
        seed = rng.randbytes(length)
        k, c, ok = model.bip32_master(N, seed)
        assert ok == 1 and (k, c) == bip32_model.master(seed)
    for trial in range(12):
        k, c = 1 + rng.randrange(N - 1), rng.getrandbits(256)
        index = rng.getrandbits(31) | (model.HARDENED if trial % 2 else 0)
        pt = bip340_model.mul_g(k)
        assert model.bip32_ckd_priv(N, k, c, index, pt) == (*bip32_model.ckd_priv(k, c, index), 1)
        assert model.bip32_ckd_priv(N, k, c, index, None) == ((*bip32_model.ckd_priv(k, c, index), 1) if trial % 2 else (0, 0, 0))
        x, y, t, cc, valid = model.bip32_ckd_pub_front(N, pt[0], pt[1], c, index)
        if trial % 2:
            assert (x, y, t, cc, valid) == (model.GX, model.GY, 0, 0, 0) and bip32_model.ckd_pub(pt, c, index) is None
        else:
            q, cc_ref = bip32_model.ckd_pub(pt, c, index)
            assert valid == 1 and (x, y) == pt and cc == cc_ref and bip340_model.add(pt, bip340_model.mul_g(t)) == q
            assert model.bip32_ckd_pub_accept(q[0], q[1], 1, valid, cc) == (q[0], q[1], cc_ref, 1)
    for k in (0, N, N + 1):
        assert model.bip32_ckd_priv(N, k, 5, model.HARDENED, None) == (0, 0, 0) and bip32_model.ckd_priv(k, 5, model.HARDENED) is None
    assert model.bip32_ckd_pub_front(N, model.GX, model.GY + 1, 7, 0)[4] == 0 and model.bip32_ckd_pub_accept(1, 2, 0, 1, 3) == (0, 0, 0, 0)


def test_bip32_models_on_the_published_vectors():
    """tests/golden/bip32_vectors.json: every master key, and every chain walked level by level (the parent's point from the curve model)."""
    steps = 0
    for name, vec in golden("bip32_vectors.json").items():
        if not isinstance(vec, dict):
            continue
        k, c, ok = model.bip32_master(N, bytes.fromhex(vec["seed"]))
        assert ok == 1 and (k, c) == (int(vec["master"]["k"], 16), int(vec["master"]["c"], 16)), name
        for level in vec.get("chain", []):
            index = int(level["index"], 16)
            with_point = model.bip32_ckd_priv(N, k, c, index, bip340_model.mul_g(k))
            assert with_point == (int(level["k"], 16), int(level["c"], 16), 1), (name, level["path"])
            if index >= model.HARDENED:
                assert model.bip32_ckd_priv(N, k, c, index, None) == with_point
            k, c, _ = with_point
            steps += 1
    assert steps >= 6


def test_schnorr_models_agree_at_the_real_order():
    rng = random.Random(2)
    for trial in range(10):
        d, aux, msg = 1 + rng.randrange(N - 1), (rng.getrandbits(256) if trial % 2 else None), rng.randbytes((32, 45, 0, 77)[trial % 4])
        px, py = bip340_model.mul_g(d)
        k0 = model.schnorr_nonce(N, d, aux, px, py, msg)
        xR, yR = bip340_model.mul_g(k0)
        sig = model.schnorr_finish(N, d, k0, px, py, xR, yR, msg)
        assert sig == (*bip340_model.sign(d, msg, aux or 0), 1)
        _, r, s, _ = sig
        u1, u2, x, y, valid = model.schnorr_verify_front(N, px, r, s, msg)
        assert valid == 1 and u1 == s and u2 == (N - bip340_model.challenge(r, px, msg)) % N and (x, y) == bip340_model.lift_x(px)
        R = bip340_model.add(bip340_model.mul_g(u1), bip340_model.mul(u2, (x, y)))
        assert R[0] == r and R[1] % 2 == 0 and bip340_model.verify(px, msg, r, s)
        assert model.schnorr_verify_front(N, px, P, s, msg)[4] == 0 and model.schnorr_verify_front(N, px, r, N, msg)[4] == 0
    assert model.schnorr_nonce(N, 0, None, 1, 2, b"") == 0 and model.schnorr_nonce(N, N, None, 1, 2, b"") == 0
    assert model.schnorr_finish(N, 5, 0, 1, 2, 3, 4, b"m") == (0, 0, 0, 0)


def test_schnorr_models_on_the_published_vectors():
    """tests/golden/bip340_vectors.json (BIP-340's signing vectors): nonce and finish give the published signature, the front kernel's model accepts its ranges."""
    vectors = golden("bip340_vectors.json")["cases"]
    assert len(vectors) >= 2
    for v in vectors:
        d, px, aux, m = int(v["secret_key"], 16), int(v["public_key"], 16), int(v["aux_rand"], 16), bytes.fromhex(v["message"])
        r, s = int(v["signature"][:64], 16), int(v["signature"][64:], 16)
        pt = bip340_model.mul_g(d)
        k0 = model.schnorr_nonce(N, d, aux, pt[0], pt[1], m)
        assert model.schnorr_finish(N, d, k0, pt[0], pt[1], *bip340_model.mul_g(k0), m) == (px, r, s, 1), v["index"]
        u1, u2, x, y, valid = model.schnorr_verify_front(N, px, r, s, m)
        R = bip340_model.add(bip340_model.mul_g(u1), bip340_model.mul(u2, (x, y)))
        assert valid == 1 and R[0] == r and R[1] % 2 == 0


def test_taproot_models_agree_at_the_real_order():
    rng = random.Random(3)
    for trial in range(10):
        d, merkle = 1 + rng.randrange(N - 1), (rng.getrandbits(256) if trial % 2 else None)
        pt = bip340_model.mul_g(d)
        assert model.taproot_seckey(N, d, merkle, pt[0], pt[1]) == (*btc_model.taproot_tweak_seckey(d, merkle), 1)
        x, y, t, valid = model.tweak_front(N, pt[0], merkle)
        assert valid == 1 and (x, y) == bip340_model.lift_x(pt[0]) and t == btc_model.tap_tweak(pt[0], merkle)
        q = bip340_model.add((x, y), bip340_model.mul_g(t))
        assert (q[0], q[1] & 1) == btc_model.taproot_tweak_pubkey(pt[0], merkle)
    assert model.taproot_seckey(N, 0, None, 1, 2) == (0, 0, 0) and model.taproot_seckey(N, N, None, 1, 2) == (0, 0, 0)
    assert model.tweak_front(N, P, None) == (model.GX, model.GY, 0, 0)
    v = golden("btc_vectors.json")["bip341"]              # BIP-341's wallet vector without a script tree
    assert v["merkle_root"] is None
    x, y, t, valid = model.tweak_front(N, int(v["internal_key"], 16), None)
    q = bip340_model.add((x, y), bip340_model.mul_g(t))
    assert valid == 1 and t == int(v["tweak"], 16) and (q[0], q[1] & 1) == (int(v["output_key"], 16), v["parity"])
    v = golden("btc_tree_vectors.json")["bip341_script"]  # ... and the one with a script tree of one leaf: the leaf hash is the Merkle root
    x, y, t, valid = model.tweak_front(N, int(v["internal_key"], 16), int(v["leaf_hash"], 16))
    q = bip340_model.add((x, y), bip340_model.mul_g(t))
    assert valid == 1 and t == btc_model.tap_tweak(int(v["internal_key"], 16), int(v["leaf_hash"], 16)) and (q[0], q[1] & 1) == (int(v["output_key"], 16), v["parity"])


def test_ecdsa_models_agree_at_the_real_order():
    rng = random.Random(4)
    for trial in range(16):
        e, d, k = rng.getrandbits(256), 1 + rng.randrange(N - 1), 1 + rng.randrange(N - 1)
        x, y = bip340_model.mul_g(k)
        if trial % 4 == 3:
            x = N + rng.randrange(P - N)         # the model takes k G as given: x(k G) >= n, which no nonce one can find gives
        for low_s in (False, True):
            ref = ecdsa_recover_model.sign_recoverable(SECP, e, d, k, low_s=low_s, kG=(x, y))
            r, s, ok = model.ecdsa_sign_scalars(N, e, d, k, x)
            s, v = model.sign_recovery_id(N, x, y, s, ok, low_s)
            assert ok == 1 and (r, s, v) == ref
            assert model.x_mod_n_equals(N, x, 1, r) == 1 and model.x_mod_n_equals(N, x, 0, r) == 0 and model.x_mod_n_equals(N, x, 1, (r + 1) % N) == 0
    for trial in range(8):                                # tools/rfc6979_model.py's deterministic signing: its nonce, k G from the curve model, through both kernels' models
        e, d = rng.getrandbits(256), 1 + rng.randrange(N - 1)
        k = rfc6979_model.nonce(N, e, d)[0]
        x, y = bip340_model.mul_g(k)
        for low_s in (False, True):
            r, s, ok = model.ecdsa_sign_scalars(N, e, d, k, x)
            s, v = model.sign_recovery_id(N, x, y, s, ok, low_s)
            assert ok == 1 and (r, s, v, k) == rfc6979_model.sign(SECP, e, d, low_s=low_s)
    assert rfc6979_model.sign(SECP, 5, 0) is None and model.ecdsa_sign_scalars(N, 5, 0, 9, 1) == (0, 0, 0)
    assert model.ecdsa_sign_scalars(N, 5, 7, 9, N) == (0, 0, 0) and ecdsa_recover_model.sign_recoverable(SECP, 5, 7, 9, kG=(N, 1)) is None
    r = 12345
    d = -5 * pow(r, -1, N) % N
    assert model.ecdsa_sign_scalars(N, 5, d, 9, r) == (0, 0, 0) and ecdsa_recover_model.sign_recoverable(SECP, 5, d, 9, kG=(r, 1)) is None
    v = golden("rfc6979_p256_sha256.json")                # RFC 6979 A.2.5: the signing formulas at P-256's order, x(k G) = r taken as given
    n256, d = 0xffffffff00000000ffffffffffffffffbce6faada7179e84f3b9cac2fc632551, int(v["d"], 16)
    for case in v["cases"]:
        e = int.from_bytes(hashlib.sha256(case["message"].encode()).digest(), "big")
        assert model.ecdsa_sign_scalars(n256, e, d, int(case["k"], 16), int(case["r"], 16)) == (int(case["r"], 16), int(case["s"], 16), 1)
    assert model.sign_recovery_id(N, 1, 1, (N + 1) // 2, 1, True) == ((N - 1) // 2, 0) and model.sign_recovery_id(N, 1, 1, (N - 1) // 2, 1, True) == ((N - 1) // 2, 1)


# ---- gmod_constants
def _limbs(v):
    return [(v >> (64 * j)) & (2**64 - 1) for j in range(4)]


def test_gmod_constants_agree_with_the_library_and_the_oracle(oracle):
    """For the two built-in orders: the library's own record (the field ids of the orders, every slot ecsimd_hip_get_constant has for a field) and the
    oracle's record of the same modulus.  p30, p^-1 mod 2^30, R^3 and the flags are exposed by neither: their congruences are checked below."""
    from ecsimd_amd.engine import ORDER_FIELD, load_library
    from helpers import CURVE_PARAMS, to_int
    lib = load_library()
    for cv, fid in ORDER_FIELD.items():
        n = CURVE_PARAMS[cv]["n"]
        g = launch_probe.gmod_constants(n, prime=True)
        out = (C.c_uint64 * 4)()
        for which, name in ((0, "p"), (5, "r"), (6, "rsq"), (7, "negr"), (10, "pm2"), (11, "psqrt")):
            assert lib.ecsimd_hip_get_constant(C.c_int(fid), C.c_int(which), out) == 0
            assert list(out) == _limbs(g[name]), (cv, name)
        c = oracle.constants(oracle.register_modulus(n))
        for ours, theirs in (("p", "p"), ("r", "r_p"), ("rsq", "rsq_p"), ("negr", "pm1_r_p"), ("pm2", "p_m2")):
            assert g[ours] == to_int(c[theirs]), (cv, ours)
        assert g["mprime"] == c["mprime"]


@pytest.mark.parametrize("p", [N, cases.HALF, 0xffffffff00000000ffffffffffffffffbce6faada7179e84f3b9cac2fc632551, (1 << 255) + 1, (1 << 256) - 1])
def test_gmod_constants_satisfy_their_definitions(p):
    g = launch_probe.gmod_constants(p)
    R = 1 << 256
    assert g["p"] == p and all(0 <= g[k] < p for k in ("r", "rsq", "negr", "r3"))
    assert (g["r"] - R) % p == 0 and (g["rsq"] - R * R) % p == 0 and (g["r3"] - R ** 3) % p == 0 and (g["negr"] + R) % p == 0
    assert g["pm2"] == p - 2 and 4 * g["psqrt"] + (p + 1) % 4 == p + 1
    assert sum(v << (30 * i) for i, v in enumerate(g["p30"])) == p and all(0 <= v < 1 << 30 for v in g["p30"]) and len(g["p30"]) == 9
    assert g["pinv30"] * p % (1 << 30) == 1 and (g["mprime"] * p + 1) % (1 << 32) == 0 and 0 <= g["mprime"] < 1 << 32
    assert g["flags"] == (2 if p % 4 == 3 else 0) and launch_probe.gmod_constants(p, prime=True)["flags"] == g["flags"] | 1


# ---- what the GPU test asserts of its batches before it looks at the device
def test_every_batch_has_both_sides_of_half():
    for name, build in cases.BATCHES.items():
        batch = build(cases.HALF)
        below, above = cases.sides(batch["digest"], cases.HALF)
        assert below >= cases.MIN_SIDE and above >= cases.MIN_SIDE, (name, below, above)
        assert len(batch["digest"]) == cases.LANES


def test_every_batch_takes_the_fitted_orders():
    for name, build in cases.BATCHES.items():
        batch = build(cases.HALF)
        if not batch["free"]:
            assert name.startswith("finish")      # (schnorr_finish runs at N and HALF only)
            continue
        for n, lane, where in cases.fitted_orders(batch):
            rebuilt = build(n)
            cases.assert_placed(rebuilt, n, lane, where)
            assert rebuilt["free"] == batch["free"] and [rebuilt["digest"][i] for i in batch["free"]] == [batch["digest"][i] for i in batch["free"]], name


def test_the_zero_blocks_hold_zero_sums_and_served_neighbours():
    for n in (N, cases.HALF):
        b = cases.ckd_priv(n, True)
        got = [model.bip32_ckd_priv(n, b["k"][i], b["c"][i], b["index"][i], b["point"][i]) for i in cases.ZERO_BLOCK]
        zero = [g for j, g in enumerate(got) if j % 3 == 0 and b["digest"][cases.ZERO_BLOCK.start + j] < n]
        near = [g for j, g in enumerate(got) if j % 3 != 0 and b["digest"][cases.ZERO_BLOCK.start + j] < n]
        assert len(zero) >= 3 and all(g == (0, 0, 0) for g in zero) and len(near) >= 6 and all(g[2] == 1 and g[0] in (1, n - 1) for g in near), n
        for has_root in (False, True):
            b = cases.taproot_seckey(n, has_root)
            got = [model.taproot_seckey(n, b["d"][i], b["merkle"][i], b["xP"][i], b["yP"][i]) for i in cases.ZERO_BLOCK]
            zero = [g for j, g in enumerate(got) if j % 3 == 0 and b["digest"][cases.ZERO_BLOCK.start + j] < n]
            near = [g for j, g in enumerate(got) if j % 3 != 0 and b["digest"][cases.ZERO_BLOCK.start + j] < n]
            assert len(zero) >= 3 and all(g == (0, 0, 0) for g in zero) and len(near) >= 6 and all(g[2] == 1 and g[0] in (1, n - 1) for g in near), n
            assert {b["yP"][i] & 1 for i in cases.ZERO_BLOCK if i % 3 == 0} == {0, 1}


def test_the_public_front_batch_has_every_cause_alone_and_with_a_refused_hash():
    b, n = cases.ckd_pub_front(), cases.HALF
    seen = {}
    for i in range(cases.LANES):
        key = (b["index"][i] >= model.HARDENED, not model.on_curve(b["qx"][i], b["qy"][i]), b["digest"][i] >= n)
        seen[key] = seen.get(key, 0) + 1
    assert all(seen.get((h, o, t), 0) >= 5 for h in (False, True) for o in (False, True) for t in (False, True)), seen
