"""GPU suite: Keccak-256 (ecsimd_hip_keccak256), Ethereum addresses (ecsimd_hip_eth_address) and address recovery (ecsimd_hip_eth_recover).

Every expectation comes from tools/keccak_model.py (pinned by tests/test_keccak_cpu.py), helpers.ec_mul, or the engine's OTHER public calls chained
(scalar_mult_base, ecdsa_sign_deterministic, ecdsa_recover) -- never from the call under test.  Every lane of every batch is compared.
"""
import ctypes as C
import json
import os
import random
import sys

import numpy as np
import pytest

from helpers import CURVE_PARAMS, SECP256K1, ec_mul, ints_to_arr, arr_to_ints

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import keccak_model as model  # noqa: E402

pytestmark = pytest.mark.gpu
CV = CURVE_PARAMS[SECP256K1]
N, P = CV["n"], CV["p"]
G = (CV["gx"], CV["gy"])
OUT_AFFINE = 2
LENGTHS = [0, 1, 31, 32, 55, 64, 135, 136, 137, 200, 271, 272, 273, 1000]
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "keccak256_vectors.json")))


def up(engine, ints):
    return engine.to_device(ints_to_arr([int(x) for x in ints]))


def up8(engine, values):
    import torch
    return torch.from_numpy(np.ascontiguousarray(values, dtype=np.uint8)).to(engine.tdev)


def ints(engine, t):
    return arr_to_ints(engine.to_numpy(t))


def rows(engine, host, stride, offset, n, length):
    """`host` (bytes of n records `stride` apart) on the device `offset` bytes behind a 16-byte aligned base, as the (n, length) strided view the engine takes."""
    import torch
    raw = torch.zeros(offset + n * stride + 16, dtype=torch.uint8, device=engine.tdev)
    assert raw.data_ptr() % 16 == 0
    raw[offset:offset + len(host)] = torch.from_numpy(np.frombuffer(host, dtype=np.uint8).copy()).to(engine.tdev)
    view = raw.as_strided((n, length), (stride, 1), offset)
    assert length == 0 or view.data_ptr() == raw.data_ptr() + offset          # (torch reports no address for a view without elements)
    return view


def digests(engine, e):
    return [v.to_bytes(32, "big") for v in ints(engine, e)]


# ---- 1. keccak256 against the model
@pytest.mark.parametrize("offset, unit, extra", [(0, 8, 8), (16, 8, 0), (4, 4, 4), (0, 4, 0), (1, 1, 3), (3, 1, 0)])
def test_keccak256_equals_the_model_at_every_length_and_alignment(engine, offset, unit, extra):
    """The stride is length + extra rounded up to `unit`.  unit 8 on a base that is a multiple of 16: 8-byte loads; unit 4 (the base or the stride 4 modulo 8):
    word loads; an odd base: byte loads.  The stride is larger than the length wherever extra or the rounding makes it so -- the random bytes between two
    messages must not reach a digest -- and equal to it in the last case, where a message's first byte follows its neighbour's last."""
    rng = random.Random(1000 * offset + 10 * unit + extra)
    n = 301
    for length in LENGTHS:
        stride = (length + extra + unit - 1) // unit * unit
        if unit == 4 and offset % 8 == 0 and stride % 8 == 0:
            stride += 4
        assert stride >= length and (offset | stride) % unit == 0 and (unit != 4 or (offset | stride) % 8 == 4)
        host = bytes(rng.randrange(256) for _ in range(n * stride)) if stride else b""
        got = digests(engine, engine.keccak256(rows(engine, host, stride, offset, n, length)))
        want = [model.keccak256(host[i * stride:i * stride + length]) for i in range(n)]
        assert got == want, (length, stride, offset, [i for i in range(n) if got[i] != want[i]][:5])


@pytest.mark.parametrize("offset, stride", [(0, 304), (4, 300), (1, 299)])
def test_keccak256_with_per_lane_lengths(engine, offset, stride):
    import torch
    rng = random.Random(stride)
    n = 4096
    host = bytes(rng.randrange(256) for _ in range(n * stride))
    lens = [rng.randrange(0, stride + 1) for _ in range(n)]
    lens[:8] = [0, stride, 135, 136, 137, 272, 1, stride - 1]
    lt = torch.tensor(lens, dtype=torch.int32, device=engine.tdev)
    got = digests(engine, engine.keccak256(rows(engine, host, stride, offset, n, stride), lens=lt))
    want = [model.keccak256(host[i * stride:i * stride + lens[i]]) for i in range(n)]
    assert got == want, [i for i in range(n) if got[i] != want[i]][:5]


def test_keccak256_golden_vectors(engine):
    import torch
    by_len = {}
    for row in GOLDEN["digests"]:
        by_len.setdefault(len(row["msg"]) // 2, []).append(row)
    for length, group in by_len.items():
        host = b"".join(bytes.fromhex(r["msg"]) for r in group)
        t = torch.from_numpy(np.frombuffer(host, dtype=np.uint8).copy().reshape(len(group), length)).to(engine.tdev) if length else \
            torch.zeros((len(group), 0), dtype=torch.uint8, device=engine.tdev)
        assert [d.hex() for d in digests(engine, engine.keccak256(t))] == [r["keccak256"] for r in group], length


# ---- 2. eth_address
def host_addresses(engine, t):
    return [bytes(r) for r in engine.to_numpy(t)]


def test_eth_address_known_keys_and_golden(engine):
    keys = GOLDEN["addresses"]
    pts = [ec_mul(SECP256K1, d, G) for d in (1, 2, 3)] + [(int(a["x"], 16), int(a["y"], 16)) for a in keys]
    got = host_addresses(engine, engine.eth_address(up(engine, [p[0] for p in pts]), up(engine, [p[1] for p in pts])))
    want = ["7e5f4552091a69125d5dfcb7b8c2659029395bdf", "2b5ad5c4795c026514f8317c7a215e218dccd6cf", "6813eb9362372eef6200f3b1dbc3f819671cba69"] + [a["address"] for a in keys]
    assert [g.hex() for g in got] == want


def test_eth_address_of_random_points(engine):
    rng = random.Random(4096)
    n = 4096
    d = [rng.randrange(1, N) for _ in range(n)]
    qx, qy = engine.scalar_mult_base(SECP256K1, up(engine, d), flags=OUT_AFFINE)
    xs, ys = ints(engine, qx), ints(engine, qy)
    for i in (0, 1, n - 1):
        assert (xs[i], ys[i]) == ec_mul(SECP256K1, d[i], G)
    got = host_addresses(engine, engine.eth_address(qx, qy))
    want = [model.eth_address(x, y) for x, y in zip(xs, ys)]
    assert got == want, [i for i in range(n) if got[i] != want[i]][:5]


# ---- 3. the round trip
def signed_batch(engine, n, seed, msg_bytes=150):
    """(d, e, r, s, v) on the device: e = keccak256 of random messages, low-s deterministic signatures under random keys."""
    import torch
    g = torch.Generator(device="cpu"); g.manual_seed(seed)
    msgs = torch.randint(0, 256, (n, msg_bytes), dtype=torch.uint8, generator=g).to(engine.tdev)
    rng = random.Random(seed)
    d = up(engine, [rng.randrange(1, N) for _ in range(n)])
    e = engine.keccak256(msgs)
    r, s, v, ok = engine.ecdsa_sign_deterministic(SECP256K1, e, d, low_s=True)
    assert bool(ok.all())
    return d, e, r, s, v, msgs


def test_eth_recover_round_trip(engine):
    import torch
    n = 2048
    d, e, r, s, v, msgs = signed_batch(engine, n, 2048)
    m0 = bytes(engine.to_numpy(msgs[0]))
    assert ints(engine, e)[0] == int.from_bytes(model.keccak256(m0), "big")
    qx, qy = engine.scalar_mult_base(SECP256K1, d, flags=OUT_AFFINE)
    want = engine.eth_address(qx, qy)
    cx, cy, cok = engine.ecdsa_recover(SECP256K1, e, r, s, v)
    chain = engine.eth_address(cx, cy)
    assert bool(cok.all()) and torch.equal(cx, qx) and torch.equal(cy, qy)
    for vv in (v, v + 27):
        addr, ok = engine.eth_recover(e, r, s, vv)
        assert bool(ok.all())
        assert torch.equal(addr, want)
        assert torch.equal(addr, chain)
        addr2, kx, ky, ok2 = engine.eth_recover(e, r, s, vv, want_key=True, require_low_s=True)
        assert bool(ok2.all()) and torch.equal(addr2, want) and torch.equal(kx, cx) and torch.equal(ky, cy)
    assert host_addresses(engine, want)[5] == model.eth_address(*ec_mul(SECP256K1, ints(engine, d)[5], G))


# ---- 4. refusals
def no_point_r():
    """the smallest r >= 2 with r^3 + 7 a non-residue modulo p: no curve point has that x"""
    r = 2
    while pow(r * r * r + 7, (P - 1) // 2, P) == 1:
        r += 1
    return r


def test_eth_recover_refusals(engine):
    import torch
    n = 64
    d, e, r, s, v, _ = signed_batch(engine, n, 64)
    ri, si, vi = ints(engine, r), ints(engine, s), [int(b) for b in engine.to_numpy(v)]
    assert all(x in (0, 1) for x in vi) and all(x <= N // 2 for x in si)
    cx, cy, _ = engine.ecdsa_recover(SECP256K1, e, r, s, v)
    good = host_addresses(engine, engine.eth_address(cx, cy))
    good_keys = list(zip(ints(engine, cx), ints(engine, cy)))
    bad = {}                                                              # lane -> what is wrong with it
    for lane, value in zip((3, 7, 11, 13, 17, 19), (2, 3, 4, 26, 29, 255)):
        vi[lane] = value; bad[lane] = f"v = {value}"
    ri[23] = 0; bad[23] = "r = 0"
    si[29] = 0; bad[29] = "s = 0"
    ri[31] = N; bad[31] = "r = n"
    si[37] = N; bad[37] = "s = n"
    ri[41] = no_point_r(); bad[41] = "r is no x coordinate"
    high = 43                                                             # the same signature in its high-s form: (r, n - s, v ^ 1) recovers the same key
    si[high] = N - si[high]; vi[high] ^= 1
    assert si[high] > N // 2
    vi[47] += 27                                                          # a valid neighbour in the other spelling
    rt, st, vt = up(engine, ri), up(engine, si), up8(engine, vi)
    chx, chy, chok = engine.ecdsa_recover(SECP256K1, e, rt, st, up8(engine, [x - 27 if x in (27, 28) else x & 1 for x in vi]))
    chain = host_addresses(engine, engine.eth_address(chx, chy))
    for low in (False, True):
        addr, kx, ky, ok = engine.eth_recover(e, rt, st, vt, require_low_s=low, want_key=True)
        a, okh, keys = host_addresses(engine, addr), [int(b) for b in engine.to_numpy(ok)], list(zip(ints(engine, kx), ints(engine, ky)))
        addr_only, ok_only = engine.eth_recover(e, rt, st, vt, require_low_s=low)
        assert torch.equal(addr_only, addr) and torch.equal(ok_only, ok)
        for i in range(n):
            refused = i in bad or (low and i == high)
            what = (i, bad.get(i, "high s" if i == high else "valid"), low)
            assert okh[i] == (0 if refused else 1), what
            assert a[i] == (bytes(20) if refused else good[i]), what
            assert keys[i] == ((0, 0) if refused else good_keys[i]), what
            if not refused:
                assert a[i] == chain[i], what
    assert int(engine.to_numpy(chok)[high]) == 1 and chain[high] == good[high]


# ---- 5. the chunk seam
def test_eth_recover_across_the_chunk_seam(engine):
    import torch
    base, n = 1 << 16, (1 << 22) + 3
    d, e, r, s, v, _ = signed_batch(engine, base, 65536, msg_bytes=40)
    v[5] = 2; v[base - 1] = 9                                             # refused lanes on both sides of every seam of the tiling
    reps = (n + base - 1) // base
    tile = lambda t: t.repeat((reps,) + (1,) * (t.dim() - 1))[:n].contiguous()
    E, R, S, V = tile(e), tile(r), tile(s), tile(v)
    addr, ok = engine.eth_recover(E, R, S, V)
    cx, cy, cok = engine.ecdsa_recover(SECP256K1, E, R, S, V & 1)
    accepted = ((V <= 1) | (V == 27) | (V == 28)).to(torch.uint8)
    cok = cok & accepted
    chain = engine.eth_address(cx, cy) * cok[:, None]
    assert torch.equal(ok, cok)
    assert torch.equal(addr, chain)
    assert int(ok.sum()) == n - 2 * (n // base)                           # lane 5 and the last lane of every whole tile (the 65th tile has three lanes)


# ---- 6. bad arguments
def test_bad_arguments(engine):
    import torch
    from ecsimd_amd import EcsimdHipError
    d, e, r, s, v, msgs = signed_batch(engine, 16, 16)
    engine.set_ref_square_compat(True)
    try:
        with pytest.raises(EcsimdHipError) as info:
            engine.eth_recover(e, r, s, v)
        assert "(-1)" in str(info.value) and "REF_SQUARE_COMPAT" in str(info.value)
    finally:
        engine.set_ref_square_compat(False)
    out = engine.empty(16)
    engine._bind_stream()
    lib, ptr = engine.lib, lambda t: C.c_void_p(t.data_ptr())
    rc = lib.ecsimd_hip_keccak256(engine.ctx, ptr(msgs), C.c_size_t(150), C.c_size_t(149), C.c_void_p(0), ptr(out), C.c_size_t(16))
    assert rc == -1 and b"stride_bytes" in lib.ecsimd_hip_last_error(engine.ctx)
    assert lib.ecsimd_hip_keccak256(engine.ctx, ptr(msgs), C.c_size_t((1 << 40) + 1), C.c_size_t((1 << 40) + 1), C.c_void_p(0), ptr(out), C.c_size_t(16)) == -1
    assert lib.ecsimd_hip_keccak256(engine.ctx, C.c_void_p(0), C.c_size_t(32), C.c_size_t(32), C.c_void_p(0), C.c_void_p(0), C.c_size_t(0)) == 0
    assert lib.ecsimd_hip_eth_address(engine.ctx, C.c_void_p(0), C.c_void_p(0), C.c_void_p(0), C.c_size_t(0)) == 0
    assert lib.ecsimd_hip_eth_recover(engine.ctx, C.c_void_p(0), C.c_void_p(0), C.c_void_p(0), C.c_void_p(0), C.c_void_p(0), C.c_void_p(0), C.c_void_p(0), C.c_void_p(0),
                                      C.c_size_t(0), C.c_int(0)) == 0
    assert lib.ecsimd_hip_eth_recover(engine.ctx, ptr(e), ptr(r), ptr(s), ptr(v), ptr(torch.empty(320, dtype=torch.uint8, device=engine.tdev)), C.c_void_p(0), C.c_void_p(0),
                                      ptr(engine.flags(16)), C.c_size_t(16), C.c_int(2)) == -1                       # an unknown flag
    empty = engine.keccak256(torch.zeros((0, 32), dtype=torch.uint8, device=engine.tdev))
    assert tuple(empty.shape) == (0, 4)
    addr, ok = engine.eth_recover(engine.empty(0), engine.empty(0), engine.empty(0), engine.flags(0))
    assert tuple(addr.shape) == (0, 20) and tuple(ok.shape) == (0,)
