"""GPU suite: SHA-512, HMAC-SHA-512 and BIP-32 key derivation (k_sha512.hip, k_bip32.hip).

Every expectation comes from tools/bip32_model.py (pinned to the published BIP-32 vectors and to hashlib / hmac by tests/test_bip32_cpu.py), hashlib / hmac,
or the engine's OTHER public calls (scalar_mult_base, eth_address, btc_pubkey_hash) -- never from the call under test.  Every lane of every batch is compared
unless a test says otherwise.
"""
import ctypes as C
import hashlib
import hmac
import json
import os
import random
import sys

import numpy as np
import pytest

from helpers import CURVE_PARAMS, SECP256K1, ints_to_arr, arr_to_ints

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bip32_model as model  # noqa: E402
import btc_model             # noqa: E402

pytestmark = pytest.mark.gpu
CV = CURVE_PARAMS[SECP256K1]
N, P = CV["n"], CV["p"]
OUT_AFFINE = 2
H = 1 << 31
LENGTHS = [0, 1, 111, 112, 113, 127, 128, 129, 239, 240, 256]
KEY_LENGTHS = [0, 1, 32, 127, 128, 129, 200]
KAT = json.load(open(os.path.join(ROOT, "tests", "golden", "bip32_vectors.json")))
V1 = KAT["vector1"]
V1_PATH = [int(lv["index"], 16) for lv in V1["chain"]]


def up(engine, ints):
    return engine.to_device(ints_to_arr([int(x) for x in ints]))


def ints(engine, t):
    return arr_to_ints(engine.to_numpy(t))


def flags(t):
    return [int(v) for v in t.cpu().numpy()]


def indices(engine, idx):
    import torch
    return torch.from_numpy(np.array(idx, dtype=np.uint32).view(np.int32)).to(engine.tdev)


def rows(engine, host, stride, offset, n, length):
    """`host` (bytes of n records `stride` apart) on the device `offset` bytes behind a 16-byte aligned base, as the (n, length) strided view the engine takes."""
    import torch
    raw = torch.zeros(offset + n * stride + 16, dtype=torch.uint8, device=engine.tdev)
    assert raw.data_ptr() % 16 == 0
    if host:
        raw[offset:offset + len(host)] = torch.from_numpy(np.frombuffer(host, dtype=np.uint8).copy()).to(engine.tdev)
    return raw.as_strided((n, length), (stride, 1), offset)


def digests(t):
    return [bytes(r) for r in t.cpu().numpy()]


def records(rng, n, length, unit, padded):
    """(host bytes, stride, the n messages): random bytes everywhere, between the messages as well."""
    stride = (length + (7 if padded else 0) + unit - 1) // unit * unit
    if padded and stride == length:
        stride += unit
    assert stride >= length and stride % unit == 0 and (not padded or stride > length) and (padded or unit == 4 or stride == length)
    host = rng.randbytes(n * stride)
    return host, stride, [host[i * stride:i * stride + length] for i in range(n)]


# ---- 1. the hashes
@pytest.mark.parametrize("offset, unit", [(0, 4), (4, 4), (1, 1), (3, 1)])
@pytest.mark.parametrize("padded", [True, False])
def test_sha512_and_hmac_equal_hashlib_at_every_length_and_alignment(engine, offset, unit, padded):
    """unit 4 on a base that is a multiple of 4: word loads; an odd base or stride: byte loads.  padded: the stride is larger than the length and random bytes
    lie between two messages (they must not reach a digest).  Every key length with ONE key for the call and with a key per lane, laid out like the messages."""
    rng = random.Random(512 + 100 * offset + 10 * unit + padded)
    n = 301
    for length in LENGTHS:
        host, stride, msgs = records(rng, n, length, unit, padded)
        view = rows(engine, host, stride, offset, n, length)
        assert digests(engine.sha512(view)) == [hashlib.sha512(m).digest() for m in msgs], ("sha512", length, stride)
        for klen in KEY_LENGTHS:
            khost, kstride, keys = records(rng, n, klen, unit, padded)
            one = rows(engine, keys[0], max(klen, 1), offset, 1, klen)[0]
            assert one.dim() == 1 and one.shape[0] == klen
            assert digests(engine.hmac_sha512(one, view)) == [hmac.new(keys[0], m, hashlib.sha512).digest() for m in msgs], ("one key", klen, length)
            each = rows(engine, khost, kstride, offset, n, klen)
            assert digests(engine.hmac_sha512(each, view)) == [hmac.new(k, m, hashlib.sha512).digest() for k, m in zip(keys, msgs)], ("a key per lane", klen, length)


def test_abc_as_a_lane(engine):
    want = bytes.fromhex(KAT["sha512_abc"])
    assert hashlib.sha512(b"abc").digest() == want
    assert digests(engine.sha512(rows(engine, b"abc" * 3, 3, 0, 3, 3))) == [want] * 3
    assert digests(engine.sha512(rows(engine, b"abcd" * 3, 4, 0, 3, 3))) == [want] * 3


# ---- 2. bip32_master
@pytest.mark.parametrize("length", [16, 32, 33, 64])
def test_bip32_master_on_the_published_seeds_among_random_ones(engine, length):
    rng = random.Random(3200 + length)
    published = [(bytes.fromhex(KAT[v]["seed"]), KAT[v]["master"]) for v in ("vector1", "vector2", "vector3")]
    for padded, offset in ((False, 0), (True, 3)):
        n = 130
        stride = length + (5 if padded else 0)
        host = bytearray(rng.randrange(256) for _ in range(n * stride))
        mine = [(s, m) for s, m in published if len(s) == length]
        for j, (s, _) in enumerate(mine):
            host[(7 + 40 * j) * stride:(7 + 40 * j) * stride + length] = s
        host = bytes(host)
        seeds = [host[i * stride:i * stride + length] for i in range(n)]
        k, c, ok = engine.bip32_master(rows(engine, host, stride, offset, n, length))
        want = [model.master(s) for s in seeds]
        assert all(w is not None for w in want)
        assert list(zip(ints(engine, k), ints(engine, c))) == want and flags(ok) == [1] * n
        for j, (_, m) in enumerate(mine):
            assert want[7 + 40 * j] == (int(m["k"], 16), int(m["c"], 16))
        assert length not in (16, 64) or mine


def test_bip32_master_refuses_seed_lengths_outside_16_to_64(engine):
    import torch
    from ecsimd_amd.engine import EcsimdHipError
    for bad in (15, 65):
        with pytest.raises(EcsimdHipError, match=r"\(-1\)"):
            engine.bip32_master(torch.zeros((4, bad), dtype=torch.uint8, device=engine.tdev))


# ---- 3. bip32_ckd_priv
def test_vector_1_level_by_level_and_as_a_path(engine):
    k0, c0 = int(V1["master"]["k"], 16), int(V1["master"]["c"], 16)
    n = 5
    k, c = up(engine, [k0] * n), up(engine, [c0] * n)
    for lv in V1["chain"]:
        k, c, ok = engine.bip32_ckd_priv(k, c, int(lv["index"], 16))
        assert ints(engine, k) == [int(lv["k"], 16)] * n and ints(engine, c) == [int(lv["c"], 16)] * n and flags(ok) == [1] * n, lv["path"]
    kd, cd, okd = engine.bip32_derive_priv(up(engine, [k0] * n), up(engine, [c0] * n), V1_PATH)
    last = V1["chain"][-1]
    assert ints(engine, kd) == [int(last["k"], 16)] * n and ints(engine, cd) == [int(last["c"], 16)] * n and flags(okd) == [1] * n
    # vector 3: keys with leading zero bytes
    v3 = KAT["vector3"]
    k, c, ok = engine.bip32_ckd_priv(up(engine, [int(v3["master"]["k"], 16)] * 2), up(engine, [int(v3["master"]["c"], 16)] * 2), H)
    assert ints(engine, k) == [int(v3["chain"][0]["k"], 16)] * 2 and ints(engine, c) == [int(v3["chain"][0]["c"], 16)] * 2 and flags(ok) == [1, 1]
    # a refused lane stays refused down the path, and the masks are ANDed
    kd, cd, okd = engine.bip32_derive_priv(up(engine, [k0, 0, N]), up(engine, [c0] * 3), V1_PATH)
    assert ints(engine, kd) == [int(last["k"], 16), 0, 0] and ints(engine, cd) == [int(last["c"], 16), 0, 0] and flags(okd) == [1, 0, 0]


@pytest.fixture(scope="module")
def parents():
    """257 random parents, the boundary keys and the boundary indices, with the model's children: computed once, shared, never changed."""
    rng = random.Random(3201)
    ks = [rng.randrange(1, N) for _ in range(257)]
    idx = [rng.randrange(H) if i % 2 else H + rng.randrange(H) for i in range(257)]
    ks += [rng.randrange(1, N) for _ in range(4)]; idx += [0, H - 1, H, 2**32 - 1]
    for bad in (0, N, N + 1, 2**256 - 1, N - 1, 1):
        ks += [bad, bad]; idx += [5, H + 5]
    cs = [rng.randrange(2**256) for _ in ks]
    want = [model.ckd_priv(k, c, i) for k, c, i in zip(ks, cs, idx)]
    assert want[-12:-4] == [None] * 8 and all(w is not None for w in want[:-12] + want[-4:])
    return ks, cs, idx, want


def as_rows(want):
    return [(0, 0, 0) if w is None else (w[0], w[1], 1) for w in want]


def test_ckd_priv_against_the_model_on_mixed_indices_and_boundary_keys(parents):
    """Runs on a context of its own: the context's scratch block then holds nothing but what this call used, and every byte of it is zero afterwards."""
    from ecsimd_amd import Engine
    engine = Engine(0)
    ks, cs, idx, want = parents
    k, c, ok = engine.bip32_ckd_priv(up(engine, ks), up(engine, cs), indices(engine, idx))
    ws = engine.workspace_bytes()
    assert ws.size >= len(ks) * 160 and not ws.any()
    assert list(zip(ints(engine, k), ints(engine, c), flags(ok))) == as_rows(want)
    engine.close()


def test_ckd_priv_with_the_promise_of_hardened_indices(engine, parents):
    ks, cs, idx, want = parents
    k, c, ok = engine.bip32_ckd_priv(up(engine, ks), up(engine, cs), indices(engine, idx), all_hardened=True)
    assert any(i < H and w is not None for i, w in zip(idx, want))
    assert list(zip(ints(engine, k), ints(engine, c), flags(ok))) == as_rows([w if i >= H else None for i, w in zip(idx, want)])
    # one lane that breaks the promise: that lane alone is refused, the others equal the call without the flag
    hard = [i | H for i in idx]
    base = engine.bip32_ckd_priv(up(engine, ks), up(engine, cs), indices(engine, hard))
    hard[100] = 7
    got = engine.bip32_ckd_priv(up(engine, ks), up(engine, cs), indices(engine, hard), all_hardened=True)
    for g, b in zip(got, base):
        g, b = (flags(g), flags(b)) if g.dim() == 1 else (ints(engine, g), ints(engine, b))
        assert g[100] == 0 and b[100] != 0 and g[:100] + g[101:] == b[:100] + b[101:]


@pytest.mark.parametrize("index", [0, 7, H - 1, H, H + 44, 2**32 - 1])
def test_one_index_for_the_call_equals_a_filled_index_array(engine, parents, index):
    ks, cs, _, _ = parents
    k, c = up(engine, ks), up(engine, cs)
    one = engine.bip32_ckd_priv(k, c, index)
    filled = engine.bip32_ckd_priv(k, c, indices(engine, [index] * len(ks)))
    assert ints(engine, one[0]) == ints(engine, filled[0]) and ints(engine, one[1]) == ints(engine, filled[1]) and flags(one[2]) == flags(filled[2])
    assert sum(flags(one[2])) == len(ks) - 8
    if index < H:
        qx, qy = engine.scalar_mult_base(SECP256K1, k, OUT_AFFINE)[:2]
        pub = engine.bip32_ckd_pub(qx, qy, c, index)
        arr = engine.bip32_ckd_pub(qx, qy, c, indices(engine, [index] * len(ks)))
        assert all(ints(engine, a) == ints(engine, b) for a, b in zip(pub[:3], arr[:3])) and flags(pub[3]) == flags(arr[3])


def test_the_engine_refuses_operands_of_different_lengths_and_takes_numpy_indices(engine):
    from ecsimd_amd.engine import EcsimdHipError
    k, c, short = up(engine, [3, 4, 5]), up(engine, [6, 7, 8]), up(engine, [6, 7])
    for call in (lambda: engine.bip32_ckd_priv(k, short, H), lambda: engine.bip32_ckd_pub(k, short, c, 1), lambda: engine.bip32_ckd_pub(k, k, short, 1),
                 lambda: engine.bip32_ckd_priv(k, c, indices(engine, [H, H]))):
        with pytest.raises(EcsimdHipError, match="batch length"):
            call()
    a, b = engine.bip32_ckd_priv(k, c, np.uint32(H + 1)), engine.bip32_ckd_priv(k, c, H + 1)
    assert ints(engine, a[0]) == ints(engine, b[0]) and ints(engine, engine.bip32_ckd_priv(k, c, np.arange(3)[2])[0]) == ints(engine, engine.bip32_ckd_priv(k, c, 2)[0])


def test_the_bip32_calls_refuse_bad_arguments(engine):
    k = up(engine, [3, 4, 5]); c = up(engine, [6, 7, 8]); ko = engine.empty(3); co = engine.empty(3); ok = engine.flags(3)
    p = lambda t: C.c_void_p(t.data_ptr())
    priv, pub = engine.lib.ecsimd_hip_bip32_ckd_priv, engine.lib.ecsimd_hip_bip32_ckd_pub
    tail = (C.c_size_t(3), C.c_int(0))
    assert priv(engine.ctx, p(k), p(c), None, C.c_uint32(H), p(ko), p(co), p(ok), *tail) == 0
    for args in ((k, c, k, co), (k, c, c, co), (k, c, ko, k), (k, c, ko, ko)):
        assert priv(engine.ctx, p(args[0]), p(args[1]), None, C.c_uint32(H), p(args[2]), p(args[3]), p(ok), *tail) == -1, "ERR_BAD_ARG"
    assert priv(engine.ctx, p(k), p(c), C.c_void_p(k.data_ptr() + 2), C.c_uint32(0), p(ko), p(co), p(ok), *tail) == -1, "a misaligned index"
    assert priv(engine.ctx, p(k), p(c), None, C.c_uint32(H), p(ko), p(co), p(ok), C.c_size_t(3), C.c_int(2)) == -1, "an unknown flag"
    assert priv(engine.ctx, None, p(c), None, C.c_uint32(H), p(ko), p(co), p(ok), *tail) == -1, "a null pointer"
    assert priv(engine.ctx, C.c_void_p(k.data_ptr() + 8), p(c), None, C.c_uint32(H), p(ko), p(co), p(ok), *tail) == -1, "a misaligned key"
    assert priv(engine.ctx, None, None, None, C.c_uint32(1), None, None, None, C.c_size_t(0), C.c_int(0)) == 0, "n = 0"
    assert pub(engine.ctx, p(k), p(c), p(c), None, C.c_uint32(1), p(ko), p(co), p(k), p(ok), C.c_size_t(3)) == -1, "an output aliasing an input"
    engine.set_ref_square_compat(True)
    try:
        seed = engine.torch.zeros(48, dtype=engine.torch.uint8, device=engine.tdev)
        assert priv(engine.ctx, p(k), p(c), None, C.c_uint32(H), p(ko), p(co), p(ok), *tail) == -1
        assert pub(engine.ctx, p(k), p(c), p(c), None, C.c_uint32(1), p(ko), p(co), p(engine.empty(3)), p(ok), C.c_size_t(3)) == -1
        assert engine.lib.ecsimd_hip_bip32_master(engine.ctx, p(seed), C.c_size_t(16), C.c_size_t(16), p(ko), p(co), p(ok), C.c_size_t(3)) == -1
    finally:
        engine.set_ref_square_compat(False)


# ---- 4. bip32_ckd_pub
def test_ckd_pub_of_the_public_key_is_the_public_key_of_ckd_priv(engine, parents):
    rng = random.Random(3202)
    ks, cs = parents[0][:257], parents[1][:257]
    idx = [rng.randrange(H) for _ in ks[:253]] + [0, 1, H - 2, H - 1]
    k, c, index = up(engine, ks), up(engine, cs), indices(engine, idx)
    qx, qy = engine.scalar_mult_base(SECP256K1, k, OUT_AFFINE)[:2]
    kc, cc, ok = engine.bip32_ckd_priv(k, c, index)
    wx, wy = engine.scalar_mult_base(SECP256K1, kc, OUT_AFFINE)[:2]
    cx, cy, pc, pok = engine.bip32_ckd_pub(qx, qy, c, index)
    assert flags(ok) == [1] * len(ks) == flags(pok)
    assert ints(engine, cx) == ints(engine, wx) and ints(engine, cy) == ints(engine, wy) and ints(engine, pc) == ints(engine, cc)
    # the model on a sample: its curve arithmetic is Python's
    xs, ys, gx, gy, gc = ints(engine, qx), ints(engine, qy), ints(engine, cx), ints(engine, cy), ints(engine, pc)
    for i in list(range(0, 257, 16)) + [253, 254, 255, 256]:
        assert model.ckd_pub((xs[i], ys[i]), cs[i], idx[i]) == ((gx[i], gy[i]), gc[i]), i


def test_ckd_pub_refuses_hardened_indices_and_points_off_the_curve(engine, parents):
    ks, cs = parents[0][:40], parents[1][:40]
    qx, qy = engine.scalar_mult_base(SECP256K1, up(engine, ks), OUT_AFFINE)[:2]
    xs, ys = ints(engine, qx), ints(engine, qy)
    idx = [5] * 40
    for i in (3, 4, 5):
        idx[i] = (H, H + 9, 2**32 - 1)[i - 3]
    ys[10] ^= 1                     # off the curve
    xs[11], ys[11] = 0, 0
    ys[13] = P - ys[13]             # the opposite point: on the curve, served
    # qx >= p and qy >= p on their own: p is within 2^32 + 977 of 2^256, so only a point with a coordinate below that can be handed in as coordinate + p.
    # (1, sqrt(8)) and (cbrt(-6), 1) are such points: lanes 15 and 16 serve them as they are, lanes 12 and 14 hold the same residues, refused by the range check alone.
    y1 = pow(8, (P + 1) // 4, P)
    x1 = pow(P - 6, (P + 2) // 9, P)                                           # p = 7 mod 9: a cube's root is its ((p + 2) / 9)-th power
    assert y1 * y1 % P == 8 and pow(x1, 3, P) == P - 6 and model.on_curve(1, y1) and model.on_curve(x1, 1) and 1 + P < 2**256
    xs[15], ys[15] = 1, y1
    xs[16], ys[16] = x1, 1
    xs[12], ys[12] = 1 + P, y1
    xs[14], ys[14] = x1, 1 + P
    bad = {3, 4, 5, 10, 11, 12, 14}
    want = [None if i in bad else model.ckd_pub((xs[i], ys[i]), cs[i], idx[i]) for i in range(40)]
    assert all(model.ckd_pub((xs[i], ys[i]), cs[i], idx[i]) is None for i in bad) and sum(w is not None for w in want) == 33
    cx, cy, cc, ok = engine.bip32_ckd_pub(up(engine, xs), up(engine, ys), up(engine, cs), indices(engine, idx))
    got = list(zip(ints(engine, cx), ints(engine, cy), ints(engine, cc), flags(ok)))
    assert got == [(0, 0, 0, 0) if w is None else (w[0][0], w[0][1], w[1], 1) for w in want]


# ---- 5. end to end
def test_from_a_seed_to_deposit_addresses(engine):
    """seed -> master -> m/44'/60'/0'/0 -> 256 last indices -> public keys -> Ethereum addresses and Bitcoin key hashes, all against the model's chain on the
    host; and the parent fingerprint BIP-32 publishes for m/0' of vector 1."""
    import keccak_model
    n = 256
    seed = bytes.fromhex(KAT["vector2"]["seed"])
    path = [H + 44, H + 60, H, 0]
    k, c, ok = engine.bip32_master(rows(engine, seed * n, 64, 0, n, 64))
    k, c, okd = engine.bip32_derive_priv(k, c, path)
    k, c, okl = engine.bip32_ckd_priv(k, c, indices(engine, list(range(n))))
    assert flags(ok) == flags(okd) == flags(okl) == [1] * n
    qx, qy = engine.scalar_mult_base(SECP256K1, k, OUT_AFFINE)[:2]
    mk, mc = model.derive(*model.master(seed), path)
    leaves = [model.ckd_priv(mk, mc, i) for i in range(n)]
    assert list(zip(ints(engine, k), ints(engine, c))) == leaves
    pts = [model.mul_g(leaf[0]) for leaf in leaves]
    assert list(zip(ints(engine, qx), ints(engine, qy))) == pts
    assert digests(engine.eth_address(qx, qy)) == [keccak_model.eth_address(x, y) for x, y in pts]
    assert digests(engine.btc_pubkey_hash(qx, qy)) == [btc_model.btc_pubkey_hash(x, y) for x, y in pts]
    # watch-only: the same leaves from the account's public key
    ax, ay = engine.scalar_mult_base(SECP256K1, up(engine, [mk] * n), OUT_AFFINE)[:2]
    cx, cy, cc, pok = engine.bip32_ckd_pub(ax, ay, up(engine, [mc] * n), indices(engine, list(range(n))))
    assert list(zip(ints(engine, cx), ints(engine, cy))) == pts and ints(engine, cc) == [leaf[1] for leaf in leaves] and flags(pok) == [1] * n
    m0 = up(engine, [int(V1["master"]["k"], 16)])
    mx, my = engine.scalar_mult_base(SECP256K1, m0, OUT_AFFINE)[:2]
    assert model.ser_p((ints(engine, mx)[0], ints(engine, my)[0])).hex() == V1["master_pubkey"]
    assert digests(engine.btc_pubkey_hash(mx, my))[0][:4].hex() == V1["master_fingerprint"] == model.fingerprint(int(V1["master"]["k"], 16)).hex()


# ---- 6. one chunk boundary
def test_ckd_priv_and_ckd_pub_across_the_chunk_boundary(engine):
    """2^22 + 5 distinct random parents with non-hardened indices: CKDpub of k G equals the public key of CKDpriv of k, with the same chain code, on EVERY lane
    (compared on the device).  The model is asked for lanes 0, 2^22 - 1, 2^22, n - 1 and 60 seeded random ones only: its curve arithmetic is Python's, a few
    milliseconds per lane."""
    import torch
    n = (1 << 22) + 5
    g = torch.Generator(device=engine.tdev); g.manual_seed(3203)
    k = torch.randint(-2**63, 2**63 - 1, (n, 4), dtype=torch.int64, device=engine.tdev, generator=g)
    c = torch.randint(-2**63, 2**63 - 1, (n, 4), dtype=torch.int64, device=engine.tdev, generator=g)
    index = torch.randint(0, 2**31 - 1, (n,), dtype=torch.int32, device=engine.tdev, generator=g)
    kc, cc, ok = engine.bip32_ckd_priv(k, c, index)
    assert bool(ok.all())                                                          # a random 256-bit key is below n but for 2^-128
    qx, qy = engine.scalar_mult_base(SECP256K1, k, OUT_AFFINE)[:2]
    cx, cy, pc, pok = engine.bip32_ckd_pub(qx, qy, c, index)
    wx, wy = engine.scalar_mult_base(SECP256K1, kc, OUT_AFFINE)[:2]
    assert bool(pok.all()) and bool((cx == wx).all()) and bool((cy == wy).all()) and bool((pc == cc).all())
    rng = random.Random(3204)
    lanes = [0, (1 << 22) - 1, 1 << 22, n - 1] + [rng.randrange(n) for _ in range(60)]
    pick = lambda t: engine.select_rows(t, np.array(lanes))
    ks, cs, idx = ints(engine, pick(k)), ints(engine, pick(c)), [int(v) for v in index[torch.tensor(lanes, device=engine.tdev)].cpu().numpy()]
    got = list(zip(ints(engine, pick(kc)), ints(engine, pick(cc))))
    assert got == [model.ckd_priv(a, b, i) for a, b, i in zip(ks, cs, idx)]
