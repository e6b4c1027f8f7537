"""GPU suite: SHA-256 on the device (ecsimd_hip_sha256), the RFC 6979 nonce (ecsimd_hip_rfc6979_nonce) and deterministic signing
(ecsimd_hip_ecdsa_sign_deterministic).

Expected values come from hashlib, from the host model on Python integers, hmac and hashlib (tools/rfc6979_model.py, pinned to the known answers of
RFC 6979 A.2.5 by tests/test_ecdsa_deterministic_cpu.py), from libcrypto, and from the engine's OTHER public calls chained (rfc6979_nonce ->
ecdsa_sign_recoverable), which must give the same bits.
"""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

from helpers import CURVE_PARAMS, P256, SECP256K1, to_int, ints_to_arr, arr_to_ints

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import rfc6979_model as model  # noqa: E402

pytestmark = pytest.mark.gpu
THREADS = 16
BUILT_IN = ["p256", "secp256k1"]
NAMED_CURVES = ["brainpoolP256r1", "sm2", "frp256v1"]
GENERIC = ["p256-generic", "secp256k1-generic"]
ALL = BUILT_IN + NAMED_CURVES + GENERIC
CHUNK = 1 << 22                     # the signing path's chunk: what ecdsa_sign_recoverable takes at a time on a registered curve
COMB_CT = 2 | 4 | 128               # OUT_AFFINE | ALG_WINDOWED | ALG_CONSTANT_TIME


def curve_of(name):
    """(id, parameters) of a curve name; '<built-in>-generic' registers the built-in curve like any other (ECSIMD_HIP_CURVE_GENERIC_KERNELS)."""
    from ecsimd_amd.curves import NAMED, curve_id
    from ecsimd_amd.engine import register_curve
    if name.endswith("-generic"):
        c = dict(CURVE_PARAMS[P256 if name.startswith("p256") else SECP256K1]); c["a"] %= c["p"]
        return register_curve(c["p"], c["a"], c["b"], c["gx"], c["gy"], c["n"], generic_kernels=True), c
    cid = curve_id(name)
    return cid, (CURVE_PARAMS[cid] if name in BUILT_IN else NAMED[name])


def up(engine, ints):
    return engine.to_device(ints_to_arr([int(x) for x in ints]))


def ints(engine, t):
    return arr_to_ints(engine.to_numpy(t))


def random_pairs(seed, n, order):
    rng = np.random.default_rng(seed)
    e = arr_to_ints(rng.integers(0, 2**64, size=(n, 4), dtype=np.uint64))
    d = [to_int(x) % (order - 1) + 1 for x in rng.integers(0, 2**64, size=(n, 4), dtype=np.uint64)]
    return e, d


# ---------------------------------------------------------------- 1. SHA-256 against hashlib
@pytest.mark.parametrize("length", [0, 1, 3, 32, 55, 56, 63, 64, 65, 119, 120, 128, 1000])
def test_sha256_against_hashlib(engine, length):
    import torch
    n = 1000 + 37                                                   # not a multiple of the 256-lane block
    rng = np.random.default_rng(4000 + length)
    for stride in (length, length + 5, ((length + 3) // 4) * 4 + 8):    # packed; a larger odd stride (byte loads); a larger word-aligned one
        rec = rng.integers(0, 256, size=(n, max(stride, 1)), dtype=np.uint8)
        dev = torch.from_numpy(rec).to(engine.tdev)
        got = ints(engine, engine.sha256(dev[:, :length]))
        want = [int.from_bytes(hashlib.sha256(rec[i, :length].tobytes()).digest(), "big") for i in range(n)]
        assert got == want, (length, stride)


# ---------------------------------------------------------------- 2. the nonce against the model, bit for bit
_MODEL_CACHE = {}


def model_nonces(order, e, d, key):
    if key not in _MODEL_CACHE:
        _MODEL_CACHE[key] = [model.nonce(order, a, b) for a, b in zip(e, d)]
    return _MODEL_CACHE[key]


@pytest.mark.parametrize("name", ALL)
def test_nonce_against_the_model(engine, name):
    cid, c = curve_of(name)
    order = c["n"]
    n = (1 << 16) + 5
    e, d = random_pairs(6979 + order % 1000, n, order)
    want = model_nonces(order, e, d, (order, n))
    k, ok = engine.rfc6979_nonce(cid, up(engine, e), up(engine, d))
    assert engine.to_numpy(ok).all()
    assert ints(engine, k) == [w[0] for w in want]
    rejected = [w[1] for w in want]
    if name == "brainpoolP256r1":                                   # what this test may NOT leave uncovered: the retry loop, run by a quarter of the lanes, three deep somewhere
        assert sum(1 for x in rejected if x) >= n // 4 and max(rejected) >= 3, (sum(1 for x in rejected if x), max(rejected))
    if name == "frp256v1":
        assert sum(1 for x in rejected if x) > 0


# ---------------------------------------------------------------- 3. the known answers, from the messages
def test_known_answers_through_sha256_and_deterministic_signing(engine):
    import torch
    kat = json.load(open(os.path.join(ROOT, "tests", "golden", "rfc6979_p256_sha256.json")))
    d = int(kat["d"], 16)
    for case in kat["cases"]:
        msg = case["message"].encode()
        dev = torch.from_numpy(np.frombuffer(msg, dtype=np.uint8).copy()).to(engine.tdev).reshape(1, -1)
        e = engine.sha256(dev)
        assert ints(engine, e) == [model.digest_int(msg)]
        r, s, v, ok = engine.ecdsa_sign_deterministic(P256, e, up(engine, [d]))
        assert engine.to_numpy(ok).tolist() == [1]
        assert ints(engine, r) == [int(case["r"], 16)] and ints(engine, s) == [int(case["s"], 16)]
        k, kok = engine.rfc6979_nonce(P256, e, up(engine, [d]))
        assert ints(engine, k) == [int(case["k"], 16)] and engine.to_numpy(kok).tolist() == [1]


# ---------------------------------------------------------------- 4. deterministic signing = the chain; the signatures verify; the key comes back
@pytest.mark.parametrize("name", ALL)
def test_deterministic_signing_equals_the_chain(engine, openssl, name):
    cid, c = curve_of(name)
    order = c["n"]
    n = 4096 + 3
    e, d = random_pairs(7000 + order % 1000, n, order)
    E, D = up(engine, e), up(engine, d)
    qx, qy = engine.scalar_mult_base(cid, D, flags=COMB_CT)[:2]
    k, kok = engine.rfc6979_nonce(cid, E, D)
    assert engine.to_numpy(kok).all()
    for low_s in (False, True):
        r, s, v, ok = engine.ecdsa_sign_deterministic(cid, E, D, low_s=low_s)
        cr, cs, cv, cok = engine.ecdsa_sign_recoverable(cid, E, D, k, low_s=low_s)
        for a, b in ((r, cr), (s, cs), (v, cv), (ok, cok)):
            assert np.array_equal(engine.to_numpy(a), engine.to_numpy(b)), (name, low_s)
        assert engine.to_numpy(ok).all()
        if low_s:
            assert all(x <= order // 2 for x in ints(engine, s))
        assert engine.to_numpy(engine.ecdsa_verify(cid, E, r, s, qx, qy)).all()
        rx, ry, rok = engine.ecdsa_recover(cid, E, r, s, v)
        assert engine.to_numpy(rok).all() and np.array_equal(engine.to_numpy(rx), engine.to_numpy(qx)) and np.array_equal(engine.to_numpy(ry), engine.to_numpy(qy))
        if name in BUILT_IN:                                        # an independent verifier on a sample
            m = 512
            assert openssl.ecdsa_verify(cid, ints_to_arr(e[:m]), engine.to_numpy(r)[:m], engine.to_numpy(s)[:m], engine.to_numpy(qx)[:m], engine.to_numpy(qy)[:m], threads=THREADS).all()
        for i in range(0, n, 257):                                  # and the model, r, s and v included
            assert (ints(engine, r)[i], ints(engine, s)[i], int(engine.to_numpy(v)[i])) == model.sign(c, e[i], d[i], low_s=low_s)[:3]


# ---------------------------------------------------------------- 5. edges, each lane against the model
@pytest.mark.parametrize("name", ALL)
def test_edges_against_the_model(engine, name):
    cid, c = curve_of(name)
    order = c["n"]
    es = [0, order - 1, order, order + 1, 2**256 - 1]
    ds = [0, 1, order - 1, order, 2**256 - 1]
    e = [a for a in es for _ in ds] + [0x1234 << 200]
    d = [b for _ in es for b in ds] + [7]
    E, D = up(engine, e), up(engine, d)
    k, kok = engine.rfc6979_nonce(cid, E, D)
    want = [model.nonce(order, a, b) for a, b in zip(e, d)]
    assert ints(engine, k) == [0 if w is None else w[0] for w in want]
    assert engine.to_numpy(kok).tolist() == [0 if w is None else 1 for w in want]
    assert [w is None for w in want] == [not 1 <= b < order for b in d]
    for low_s in (False, True):
        sig = [model.sign(c, a, b, low_s=low_s) for a, b in zip(e, d)]
        r, s, v, ok = engine.ecdsa_sign_deterministic(cid, E, D, low_s=low_s)
        assert ints(engine, r) == [0 if w is None else w[0] for w in sig]
        assert ints(engine, s) == [0 if w is None else w[1] for w in sig]
        assert engine.to_numpy(v).tolist() == [0 if w is None else w[2] for w in sig]
        assert engine.to_numpy(ok).tolist() == [0 if w is None else 1 for w in sig]
        r2, s2, none, ok2 = engine.ecdsa_sign_deterministic(cid, E, D, low_s=low_s, want_v=False)       # v = NULL
        assert none is None
        for a, b in ((r, r2), (s, s2), (ok, ok2)):
            assert np.array_equal(engine.to_numpy(a), engine.to_numpy(b))
    # n = 1
    r, s, v, ok = engine.ecdsa_sign_deterministic(cid, E[-1:].contiguous(), D[-1:].contiguous())
    one = model.sign(c, e[-1], d[-1])
    assert (ints(engine, r)[0], ints(engine, s)[0], int(engine.to_numpy(v)[0]), int(engine.to_numpy(ok)[0])) == (*one[:3], 1)
    # n = 0
    empty = engine.empty(0)
    assert engine.ecdsa_sign_deterministic(cid, empty, empty)[0].shape[0] == 0 and engine.rfc6979_nonce(cid, empty, empty)[0].shape[0] == 0


def test_unsupported_curves_are_refused(engine):
    from ecsimd_amd.engine import EcsimdHipError, register_curve
    c = __import__("ecsimd_amd.curves", fromlist=["NAMED"]).NAMED["sm2"]
    no_order = register_curve(c["p"], c["a"], c["b"], c["gx"], c["gy"], None)
    one = up(engine, [5])
    for call in (lambda: engine.rfc6979_nonce(no_order, one, one), lambda: engine.ecdsa_sign_deterministic(no_order, one, one),
                 lambda: engine.rfc6979_nonce(12345, one, one)):
        with pytest.raises(EcsimdHipError):
            call()


# ---------------------------------------------------------------- 6. across the chunk boundary, and what the workspace holds afterwards
@pytest.mark.parametrize("name", ["secp256k1", "brainpoolP256r1"])
def test_a_batch_that_crosses_the_chunk_boundary_by_three(engine, name):
    import torch
    cid, c = curve_of(name)
    order = c["n"]
    n = CHUNK + 3
    g = torch.Generator(device="cpu"); g.manual_seed(99)
    E = torch.randint(-2**63, 2**63 - 1, (n, 4), dtype=torch.int64, generator=g).to(engine.tdev)
    D = torch.randint(-2**63, 2**63 - 1, (n, 4), dtype=torch.int64, generator=g)
    D[:, 3] &= 0x3fffffffffffffff                                   # d < 2^254 < n; and not zero (a 254-bit random value)
    D = D.to(engine.tdev)
    r, s, v, ok = engine.ecdsa_sign_deterministic(cid, E, D, low_s=True)
    k, kok = engine.rfc6979_nonce(cid, E, D)
    assert bool(kok.all()) and bool(ok.all())
    # the chain, one chunk at a time (a registered curve's ecdsa_sign_recoverable takes 2^22)
    for lo, hi in ((0, CHUNK), (CHUNK, n)):
        cr, cs, cv, cok = engine.ecdsa_sign_recoverable(cid, E[lo:hi].contiguous(), D[lo:hi].contiguous(), k[lo:hi].contiguous(), low_s=True)
        assert torch.equal(cr, r[lo:hi]) and torch.equal(cs, s[lo:hi]) and torch.equal(cv, v[lo:hi]) and torch.equal(cok, ok[lo:hi])
    rows = [0, 1, CHUNK - 2, CHUNK - 1, CHUNK, CHUNK + 1, CHUNK + 2]
    e_i, d_i = ints(engine, engine.select_rows(E, rows)), ints(engine, engine.select_rows(D, rows))
    got = list(zip(ints(engine, engine.select_rows(r, rows)), ints(engine, engine.select_rows(s, rows)), engine.to_numpy(v.cpu()[rows]).tolist(),
                   ints(engine, engine.select_rows(k, rows))))
    assert got == [model.sign(c, a, b, low_s=True) for a, b in zip(e_i, d_i)]
    # nothing of K, V, the candidates, the nonce or k G is left in the workspace
    held = CHUNK * ((160 if name in BUILT_IN else 290) + 130)       # ecdsa_sign_recoverable's part, then the nonce, K, V, the retry bytes and the spare v
    ws = engine.workspace_bytes()
    assert ws.size >= held and not ws[:held].any()


def test_the_workspace_is_zero_after_a_small_call(engine):
    cid, c = curve_of("frp256v1")
    e, d = random_pairs(31, 3000, c["n"])
    engine.ecdsa_sign_deterministic(cid, up(engine, e), up(engine, d))
    assert not engine.workspace_bytes()[:3000 * 420].any()
    engine.rfc6979_nonce(cid, up(engine, e), up(engine, d))
    assert not engine.workspace_bytes()[:3000 * 130].any()
