"""GPU suite: RIPEMD-160, HASH160, double SHA-256, public-key hashes and the BIP-341 Taproot key tweaks (k_btc.hip).

Every expectation comes from tools/btc_model.py (pinned to published known answers by tests/test_btc_cpu.py), hashlib, or the engine's OTHER public calls
(sha256, sec1_encode, scalar_mult_base, schnorr_sign, schnorr_verify) -- never from the call under test.  Every lane of every batch is compared.
"""
import ctypes as C
import hashlib
import json
import os
import random
import sys

import numpy as np
import pytest

from helpers import CURVE_PARAMS, SECP256K1, ints_to_arr, arr_to_ints

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import btc_model as model  # noqa: E402

pytestmark = pytest.mark.gpu
CV = CURVE_PARAMS[SECP256K1]
N, P = CV["n"], CV["p"]
OUT_AFFINE = 2
LENGTHS = [0, 1, 31, 32, 33, 54, 55, 56, 63, 64, 65, 119, 120, 128, 200]
KAT = json.load(open(os.path.join(ROOT, "tests", "golden", "btc_vectors.json")))
RMD_KAT = [((v["msg"] * v["repeat"]).encode(), v["digest"]) for v in KAT["ripemd160"] if v["repeat"] <= 8]
H160_KAT = [(bytes.fromhex(v["msg_hex"]), v["digest"]) for v in KAT["hash160"]]


def up(engine, ints):
    return engine.to_device(ints_to_arr([int(x) for x in ints]))


def ints(engine, t):
    return arr_to_ints(engine.to_numpy(t))


def flags(t):
    return [int(v) for v in t.cpu().numpy()]


def rows(engine, host, stride, offset, n, length):
    """`host` (bytes of n records `stride` apart) on the device `offset` bytes behind a 16-byte aligned base, as the (n, length) strided view the engine takes."""
    import torch
    raw = torch.zeros(offset + n * stride + 16, dtype=torch.uint8, device=engine.tdev)
    assert raw.data_ptr() % 16 == 0
    raw[offset:offset + len(host)] = torch.from_numpy(np.frombuffer(host, dtype=np.uint8).copy()).to(engine.tdev)
    return raw.as_strided((n, length), (stride, 1), offset)


def digests20(t):
    return [bytes(r) for r in t.cpu().numpy()]


def digests32(engine, e):
    return [v.to_bytes(32, "big") for v in ints(engine, e)]


# ---- 1. the three hashes
@pytest.mark.parametrize("offset, unit", [(0, 4), (4, 4), (1, 1), (3, 1)])
@pytest.mark.parametrize("padded", [True, False])
def test_the_hashes_equal_the_model_at_every_length_and_alignment(engine, offset, unit, padded):
    """unit 4 on a base that is a multiple of 4: word loads; an odd base or stride: byte loads.  padded: the stride is larger than the length and random bytes
    lie between two messages (they must not reach a digest); else stride = length (rounded up to the unit where word loads are being tested)."""
    rng = random.Random(100 * offset + 10 * unit + padded)
    n = 301
    for length in LENGTHS:
        stride = (length + (7 if padded else 0) + unit - 1) // unit * unit
        if padded and stride == length:
            stride += unit
        assert stride >= length and (offset | stride) % unit == 0 and (not padded or stride > length) and (padded or unit == 4 or stride == length)
        host = bytearray(rng.randrange(256) for _ in range(n * stride))
        kats = [m for m, _ in RMD_KAT + H160_KAT if len(m) == length]
        for i, m in enumerate(kats):
            host[i * stride:i * stride + length] = m
        host = bytes(host)
        msgs = [host[i * stride:i * stride + length] for i in range(n)]
        view = rows(engine, host, stride, offset, n, length)
        assert digests20(engine.ripemd160(view)) == [model.ripemd160(m) for m in msgs], ("ripemd160", length, stride)
        assert digests20(engine.hash160(view)) == [model.hash160(m) for m in msgs], ("hash160", length, stride)
        dd = digests32(engine, engine.sha256d(view))
        assert dd == [hashlib.sha256(hashlib.sha256(m).digest()).digest() for m in msgs], ("sha256d", length, stride)
        once = engine.to_bytes_be(engine.sha256(view)).reshape(n, 32)
        assert dd == digests32(engine, engine.sha256(once)), ("sha256 of sha256", length)


def test_the_published_vectors_as_lanes(engine):
    for kat, call, fn in ((RMD_KAT, engine.ripemd160, model.ripemd160), (H160_KAT, engine.hash160, model.hash160)):
        for m, want in kat:
            host = m * 3
            got = digests20(call(rows(engine, host, len(m), 0, 3, len(m))))
            assert got == [bytes.fromhex(want)] * 3 and fn(m).hex() == want, m


# ---- 2. public-key hashes
def test_btc_pubkey_hash_is_hash160_of_the_sec1_encoding(engine):
    rng = random.Random(341)
    ks = [1] + [rng.randrange(1, N) for _ in range(257)]
    qx, qy = engine.scalar_mult_base(SECP256K1, up(engine, ks), OUT_AFFINE)[:2]
    xs, ys = ints(engine, qx), ints(engine, qy)
    assert (xs[0], ys[0]) == (CV["gx"], CV["gy"])
    assert any(y & 1 for y in ys) and any(not y & 1 for y in ys)
    for compressed in (True, False):
        got = digests20(engine.btc_pubkey_hash(qx, qy, compressed=compressed))
        enc = engine.sec1_encode(SECP256K1, qx, qy, compressed=compressed).reshape(len(ks), 33 if compressed else 65)
        assert got == digests20(engine.hash160(enc)), compressed
        assert got == [model.btc_pubkey_hash(x, y, compressed) for x, y in zip(xs, ys)], compressed
    assert got[0].hex() == KAT["hash160"][1]["digest"] and digests20(engine.btc_pubkey_hash(qx, qy))[0].hex() == KAT["hash160"][0]["digest"]
    zero = up(engine, [0, 0, 0])
    assert digests20(engine.btc_pubkey_hash(zero, zero)) == [model.hash160(b"\x02" + bytes(32))] * 3
    assert digests20(engine.btc_pubkey_hash(zero, zero, compressed=False)) == [model.hash160(b"\x04" + bytes(64))] * 3


# ---- 3. xonly_tweak_add
def lifting_keys(rng, count):
    out = []
    while len(out) < count:
        x = rng.randrange(P)
        if model.lift_x(x):
            out.append(x)
    return out


def check_tweaks(engine, got, want):
    qx, parity, ok = ints(engine, got[0]), flags(got[1]), flags(got[2])
    for i, w in enumerate(want):
        assert (qx[i], parity[i], ok[i]) == ((0, 0, 0) if w is None else (w[0], w[1], 1)), i


def test_xonly_tweak_add_on_random_and_crafted_lanes(engine):
    rng = random.Random(3410)
    px = lifting_keys(rng, 150) + [rng.randrange(P) for _ in range(50)]
    t = [rng.randrange(N) for _ in px]
    d = next(k for k in range(7, 99) if model.mul_g(k)[1] % 2 == 0)          # P = d G with an even y
    dx = model.mul_g(d)[0]
    key = px[0]
    crafted = [(key, 0), (key, N - 1), (key, N), (key, 2**256 - 1), (P, 5), (P + 1, 5), (2**256 - 1, 5), (5, 9), (dx, d), (dx, N - d), (CV["gx"], 1), (CV["gx"], 0), (CV["gx"], N - 1)]
    px += [c[0] for c in crafted]; t += [c[1] for c in crafted]
    want = [model.xonly_tweak_add(a, b) for a, b in zip(px, t)]
    base = len(px) - len(crafted)
    assert want[base] == (key, 0) and want[base + 1] is not None and want[base + 2] is None and want[base + 3] is None and want[base + 7] is None
    assert want[base + 8] == (model.mul_g(2 * d)[0], model.mul_g(2 * d)[1] & 1) and want[base + 9] is None and want[base + 12] is None
    assert sum(w is None for w in want) >= 10 and sum(w is not None for w in want) >= 150
    check_tweaks(engine, engine.xonly_tweak_add(up(engine, px), up(engine, t)), want)


# ---- 4. taproot_tweak_pubkey
def test_taproot_tweak_pubkey_against_the_model_and_bip341(engine):
    rng = random.Random(3411)
    v = KAT["bip341"]
    px = [int(v["internal_key"], 16)] + lifting_keys(rng, 140) + [rng.randrange(P) for _ in range(60)] + [5, P, 2**256 - 1]
    roots = [rng.randrange(2**256) for _ in px]
    want = [model.taproot_tweak_pubkey(x) for x in px]
    assert want[0] == (int(v["output_key"], 16), v["parity"]) and model.tap_tweak(px[0]) == int(v["tweak"], 16)
    assert want[-1] is None and want[-2] is None and want[-3] is None
    assert {w[1] for w in want if w} == {0, 1}
    check_tweaks(engine, engine.taproot_tweak_pubkey(up(engine, px)), want)
    want = [model.taproot_tweak_pubkey(x, h) for x, h in zip(px, roots)]
    assert {w[1] for w in want if w} == {0, 1}
    check_tweaks(engine, engine.taproot_tweak_pubkey(up(engine, px), up(engine, roots)), want)


def test_taproot_tweak_pubkey_across_the_chunk_boundary(engine):
    """2^22 + 3 lanes tiled from 1 000 distinct inputs: the model computes 1 000, every lane is compared on the device side by tiling the expectation."""
    import torch
    rng = random.Random(3412)
    distinct, n = 1000, (1 << 22) + 3
    px = lifting_keys(rng, 900) + [rng.randrange(P) for _ in range(100)]
    roots = [rng.randrange(2**256) for _ in px]
    want = [model.taproot_tweak_pubkey(x, h) for x, h in zip(px, roots)]
    reps = (n + distinct - 1) // distinct
    tile = lambda t: t.repeat((reps,) + (1,) * (t.dim() - 1))[:n].contiguous()
    qx, parity, ok = engine.taproot_tweak_pubkey(tile(up(engine, px)), tile(up(engine, roots)))
    wx = tile(up(engine, [w[0] if w else 0 for w in want]))
    wp = tile(torch.tensor([w[1] if w else 0 for w in want], dtype=torch.uint8, device=engine.tdev))
    wo = tile(torch.tensor([1 if w else 0 for w in want], dtype=torch.uint8, device=engine.tdev))
    assert qx.shape[0] == n and bool((qx == wx).all()) and bool((parity == wp).all()) and bool((ok == wo).all())
    assert int(wo[-3:].sum()) >= 1                                                # the three lanes behind the boundary hold accepted keys


# ---- 5. taproot_tweak_seckey
def seckeys(rng, count):
    ds = [rng.randrange(1, N) for _ in range(count)]
    assert {model.mul_g(d)[1] & 1 for d in ds} == {0, 1}
    return ds


@pytest.mark.parametrize("with_root", [False, True])
def test_taproot_tweak_seckey_against_the_model_and_end_to_end(engine, with_root):
    import torch
    rng = random.Random(3413 + with_root)
    ds = seckeys(rng, 200) + [0, N, N + 1, 2**256 - 1]
    roots = [rng.randrange(2**256) for _ in ds] if with_root else None
    want = [model.taproot_tweak_seckey(d, roots[i] if roots else None) for i, d in enumerate(ds)]
    assert all(w is not None for w in want[:200]) and want[200:] == [None] * 4
    rt = up(engine, roots) if roots else None
    d_out, px, ok = engine.taproot_tweak_seckey(up(engine, ds), rt)
    ws = engine.workspace_bytes()
    assert ws.size >= len(ds) * 160 and not ws[:len(ds) * 160].any()             # the Jacobian and the affine d G, 5 x 32 B per element: all the call used
    got = list(zip(ints(engine, d_out), ints(engine, px), flags(ok)))
    assert got == [(0, 0, 0) if w is None else (w[0], w[1], 1) for w in want]
    # end to end: a signature by the tweaked key verifies under the output key, which the public call makes of px
    qx, parity, qok = engine.taproot_tweak_pubkey(px, rt)
    assert flags(qok) == flags(ok)
    msgs = torch.from_numpy(np.frombuffer(bytes(rng.randrange(256) for _ in range(32 * len(ds))), dtype=np.uint8).copy()).to(engine.tdev).reshape(len(ds), 32)
    spx, r, s, sok = engine.schnorr_sign(d_out, msgs)
    assert flags(sok) == flags(ok) and ints(engine, spx) == ints(engine, qx)
    assert flags(engine.schnorr_verify(qx, msgs, r, s)) == flags(ok)
    d2, none, ok2 = engine.taproot_tweak_seckey(up(engine, ds), rt, want_px=False)
    assert none is None and ints(engine, d2) == ints(engine, d_out) and flags(ok2) == flags(ok)


def test_taproot_tweak_seckey_refuses_aliased_outputs(engine):
    d = up(engine, [3, 4, 5]); h = up(engine, [6, 7, 8]); out = engine.empty(3); px = engine.empty(3); ok = engine.flags(3)
    call = engine.lib.ecsimd_hip_taproot_tweak_seckey
    p = lambda t: C.c_void_p(t.data_ptr())
    assert call(engine.ctx, p(d), p(h), p(out), p(px), p(ok), C.c_size_t(3)) == 0
    for args in ((d, h, d, px), (d, h, h, px), (d, h, out, d), (d, h, out, h), (d, h, out, out)):
        assert call(engine.ctx, *[p(a) for a in args], p(ok), C.c_size_t(3)) == -1, "ERR_BAD_ARG"
