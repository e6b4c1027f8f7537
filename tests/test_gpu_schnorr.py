"""GPU suite: BIP-340 Schnorr signatures on the device (ecsimd_hip_schnorr_sign, ecsimd_hip_schnorr_verify).

Expected values come from the host model on Python integers and hashlib (tools/bip340_model.py, pinned to BIP-340's test vectors 0 and 1 by
tests/test_schnorr_cpu.py) and from the engine's OTHER public calls chained (sha256 -> sec1_decode -> double_scalar_mult -> comparisons on the host:
bip340_model.chain_of_existing_calls), which must give the same verdicts.
"""
import json
import os
import sys

import numpy as np
import pytest

from helpers import ints_to_arr, arr_to_ints

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bip340_model as model  # noqa: E402

pytestmark = pytest.mark.gpu
P, N = model.P, model.N
CHUNK = 1 << 22
LANES = 4096 + 5
SECP256K1 = 1
COMB_CT = 2 | 4 | 128               # OUT_AFFINE | ALG_WINDOWED | ALG_CONSTANT_TIME


def up(engine, ints):
    return engine.to_device(ints_to_arr([int(x) for x in ints]))


def ints(engine, t):
    return arr_to_ints(engine.to_numpy(t))


def flags(engine, t):
    return engine.to_numpy(t).tolist()


def messages_on_device(engine, rows, stride):
    """The messages `rows` (n, length) uint8 laid out `stride` bytes apart in a device record array filled with other bytes; returns the strided 2-D view."""
    import torch
    n, length = rows.shape
    rec = np.random.default_rng(stride).integers(0, 256, size=(n, max(stride, 1)), dtype=np.uint8)
    rec[:, :length] = rows
    return torch.from_numpy(rec).to(engine.tdev)[:, :length]


def random_keys(rng, n):
    return [int.from_bytes(rng.bytes(32), "big") % (N - 1) + 1 for _ in range(n)]


def non_curve_x(rng):
    while True:
        x = int.from_bytes(rng.bytes(32), "big") % P
        if model.lift_x(x) is None:
            return x


# ---------------------------------------------------------------- 1. the known answers
def test_known_answers_sign_and_verify(engine):
    import torch
    kat = json.load(open(os.path.join(ROOT, "tests", "golden", "bip340_vectors.json")))
    assert len(kat["cases"]) == 2
    for c in kat["cases"]:
        sig = bytes.fromhex(c["signature"])
        want = (int(c["public_key"], 16), int.from_bytes(sig[:32], "big"), int.from_bytes(sig[32:], "big"))
        msg = torch.from_numpy(np.frombuffer(bytes.fromhex(c["message"]), dtype=np.uint8).copy()).to(engine.tdev).reshape(1, -1)
        px, r, s, ok = engine.schnorr_sign(up(engine, [int(c["secret_key"], 16)]), msg, aux=up(engine, [int(c["aux_rand"], 16)]))
        assert flags(engine, ok) == [1]
        assert (ints(engine, px)[0], ints(engine, r)[0], ints(engine, s)[0]) == want
        assert flags(engine, engine.schnorr_verify(px, msg, r, s)) == [1]
        assert flags(engine, engine.schnorr_verify(up(engine, [want[0]]), msg, up(engine, [want[1]]), up(engine, [want[2]]))) == [1]
    # vector 0's aux is 32 zero bytes: aux = None signs the same
    c = kat["cases"][0]
    msg = torch.zeros((1, 32), dtype=torch.uint8, device=engine.tdev)
    px, r, s, ok = engine.schnorr_sign(up(engine, [3]), msg)
    assert ints(engine, r)[0] == int(c["signature"][:64], 16) and ints(engine, s)[0] == int(c["signature"][64:], 16) and flags(engine, ok) == [1]


# ---------------------------------------------------------------- 2. signing against the model, bit for bit
_KEYS = {}


def signing_inputs():
    if not _KEYS:
        rng = np.random.default_rng(340)
        _KEYS["d"] = random_keys(rng, LANES)
        _KEYS["aux"] = [int.from_bytes(rng.bytes(32), "big") for _ in range(LANES)]
    return _KEYS["d"], _KEYS["aux"]


@pytest.mark.parametrize("length", [32, 0, 1, 33, 55, 64, 100])
def test_sign_against_the_model(engine, length):
    d, aux = signing_inputs()
    rows = np.random.default_rng(1000 + length).integers(0, 256, size=(LANES, length), dtype=np.uint8)
    want = [model.sign(a, rows[i].tobytes(), b) for i, (a, b) in enumerate(zip(d, aux))]
    assert all(w is not None for w in want)
    D, A = up(engine, d), up(engine, aux)
    for stride in (length, length + 5, ((length + 3) // 4) * 4 + 8):        # packed; a larger odd stride (byte loads); a larger word-aligned one
        px, r, s, ok = engine.schnorr_sign(D, messages_on_device(engine, rows, stride), aux=A)
        assert all(flags(engine, ok)), (length, stride)
        assert list(zip(ints(engine, px), ints(engine, r), ints(engine, s))) == want, (length, stride)
    px, r, s, ok = engine.schnorr_sign(D, messages_on_device(engine, rows, length), aux=A, want_px=False)      # px = NULL
    assert px is None and list(zip(ints(engine, r), ints(engine, s))) == [w[1:] for w in want] and all(flags(engine, ok))


def test_sign_without_aux_is_the_model_with_zero_bytes(engine):
    d, _ = signing_inputs()
    rows = np.random.default_rng(77).integers(0, 256, size=(LANES, 32), dtype=np.uint8)
    want = [model.sign(a, rows[i].tobytes(), 0) for i, a in enumerate(d)]
    px, r, s, ok = engine.schnorr_sign(up(engine, d), messages_on_device(engine, rows, 32), aux=None)
    assert all(flags(engine, ok)) and list(zip(ints(engine, px), ints(engine, r), ints(engine, s))) == want
    px2, r2, s2, ok2 = engine.schnorr_sign(up(engine, d), messages_on_device(engine, rows, 32), aux=up(engine, [0] * LANES))
    assert ints(engine, r2) == ints(engine, r) and ints(engine, s2) == ints(engine, s)


# ---------------------------------------------------------------- 3. verification against the model, lane classes i mod 8
SUBCASES_5 = ("no point", "px >= p")
SUBCASES_7 = ("r >= p", "s >= n", "r not an x", "infinite sum")


def build_classes(rng, n, length=32):
    """(px, msgs, r, s, label) per lane, by the model: the issue's table."""
    lanes = []
    for i in range(n):
        d = random_keys(rng, 1)[0]
        msg = rng.bytes(length)
        aux = int.from_bytes(rng.bytes(32), "big")
        cls = i % 8
        label = str(cls)
        if cls == 4:                                                # R with an odd y: the nonce left as drawn, on a lane where that y is odd
            while not model.nonce_point_is_odd(d, msg, aux):
                aux += 1
            px, r, s = model.sign(d, msg, aux, negate_nonce=False)
        else:
            px, r, s = model.sign(d, msg, aux)
        if cls == 3:
            s = N - s
        elif cls == 5:
            sub = (i // 8) % 2
            label = "5:" + SUBCASES_5[sub]
            px = non_curve_x(rng) if sub == 0 else P + int.from_bytes(rng.bytes(4), "big") % (2**256 - P)
        elif cls == 6:
            m2 = bytearray(msg); bit = int.from_bytes(rng.bytes(2), "big") % (8 * length); m2[bit // 8] ^= 1 << (bit % 8); msg = bytes(m2)
        elif cls == 7:
            sub = (i // 8) % 4
            label = "7:" + SUBCASES_7[sub]
            if sub == 0:
                r = P + int.from_bytes(rng.bytes(4), "big") % (2**256 - P)
            elif sub == 1:
                s = N + int.from_bytes(rng.bytes(16), "big") % (2**256 - N)
            elif sub == 2:
                r = non_curve_x(rng)
            else:                                                   # s G = e P: the sum is the point at infinity
                r = int.from_bytes(rng.bytes(32), "big") % P
                dd = d if model.mul_g(d)[1] % 2 == 0 else N - d
                s = model.challenge(r, px, msg) * dd % N
        lanes.append((px, msg, r, s, label))
    return lanes


def test_verify_against_the_model(engine):
    rng = np.random.default_rng(3400)
    lanes = build_classes(rng, LANES)
    want = [int(model.verify(px, msg, r, s)) for px, msg, r, s, _ in lanes]
    # what the batch has to contain, by the model's own verdicts, before the device is asked
    assert sum(want) * 8 >= 3 * LANES and (LANES - sum(want)) * 2 >= LANES
    assert [w for w, lane in zip(want, lanes) if lane[4] in "012"] == [1] * sum(1 for lane in lanes if lane[4] in "012")
    assert not any(w for w, lane in zip(want, lanes) if lane[4] not in "012")
    for sub in ["5:" + x for x in SUBCASES_5] + ["7:" + x for x in SUBCASES_7]:
        assert sum(1 for lane in lanes if lane[4] == sub) >= 16, sub
    rows = np.frombuffer(b"".join(lane[1] for lane in lanes), dtype=np.uint8).reshape(LANES, 32)
    PX, R, S = up(engine, [x[0] for x in lanes]), up(engine, [x[2] for x in lanes]), up(engine, [x[3] for x in lanes])
    for stride in (32, 37, 40):
        got = flags(engine, engine.schnorr_verify(PX, messages_on_device(engine, rows, stride), R, S))
        wrong = [(i, lanes[i][4], got[i], want[i]) for i in range(LANES) if got[i] != want[i]]
        assert not wrong, wrong[:10]
    # and the public calls chained give the same verdicts
    assert model.chain_of_existing_calls(engine, PX, messages_on_device(engine, rows, 32), R, S).tolist() == want


@pytest.mark.parametrize("length", [0, 1, 33, 55, 64, 100])
def test_verify_other_message_lengths(engine, length):
    """Device-signed signatures of messages of another length verify on the device and in the model; one changed byte (or, for the empty message, one changed
    bit of s) does not."""
    n = 512 + 3
    rng = np.random.default_rng(500 + length)
    d = random_keys(rng, n)
    rows = rng.integers(0, 256, size=(n, length), dtype=np.uint8)
    msgs = messages_on_device(engine, rows, length + 3)
    px, r, s, ok = engine.schnorr_sign(up(engine, d), msgs)
    assert all(flags(engine, ok)) and all(flags(engine, engine.schnorr_verify(px, msgs, r, s)))
    for i in range(0, n, 64):
        assert model.verify(ints(engine, px)[i], rows[i].tobytes(), ints(engine, r)[i], ints(engine, s)[i])
    if length:
        rows2 = rows.copy(); rows2[:, length - 1] ^= 0x40
        assert not any(flags(engine, engine.schnorr_verify(px, messages_on_device(engine, rows2, length), r, s)))
    s2 = up(engine, [x ^ 2 for x in ints(engine, s)])
    assert not any(flags(engine, engine.schnorr_verify(px, msgs, r, s2)))


# ---------------------------------------------------------------- 4. a million lanes against the chain of existing calls
def test_verify_equals_the_chain_of_existing_calls(engine):
    import torch
    n = (1 << 20) + 3
    g = torch.Generator(device="cpu"); g.manual_seed(340)
    D = torch.randint(-2**63, 2**63 - 1, (n, 4), dtype=torch.int64, generator=g)
    D[:, 3] &= 0x3fffffffffffffff                                   # d < 2^254 < n; and not zero (a 254-bit random value)
    D = D.to(engine.tdev)
    msgs = torch.randint(0, 256, (n, 32), dtype=torch.uint8, generator=g).to(engine.tdev)
    px, r, s, ok = engine.schnorr_sign(D, msgs)
    assert bool(ok.all())
    yP = engine.scalar_mult_base(SECP256K1, D, flags=COMB_CT)[1]
    # perturb on the host: class = lane mod 8, as in the model's batch
    PX, R, S, M = (engine.to_numpy(t).copy() for t in (px, r, s, msgs.cpu()))
    d_np, y_np = engine.to_numpy(D), engine.to_numpy(yP)
    rng = np.random.default_rng(20)
    bad_x = [non_curve_x(rng) for _ in range(64)]
    one = lambda a, i: arr_to_ints(a[i:i + 1])[0]
    put = lambda a, i, v: a.__setitem__(i, ints_to_arr([v])[0])
    dprime = lambda i: one(d_np, i) if int(y_np[i, 0]) & 1 == 0 else N - one(d_np, i)
    cls = np.arange(n) % 8
    for i in np.nonzero(cls == 3)[0]:
        put(S, i, N - one(S, i))
    for i in np.nonzero(cls == 4)[0]:                               # the same x(R) with the odd y: s' = -k + e d' = 2 e d' - s
        e = model.challenge(one(R, i), one(PX, i), M[i].tobytes())
        put(S, i, (2 * e * dprime(i) - one(S, i)) % N)
    for i in np.nonzero(cls == 5)[0]:
        put(PX, i, bad_x[(i // 8) % 64] if (i // 8) % 2 == 0 else P + (int(i) * 2654435761) % (2**256 - P))
    idx6 = np.nonzero(cls == 6)[0]
    M[idx6, (idx6 // 8) % 32] ^= (1 << ((idx6 // 256) % 8)).astype(np.uint8)
    for i in np.nonzero(cls == 7)[0]:
        sub = (i // 8) % 4
        if sub == 0:
            put(R, i, P + (int(i) * 40503) % (2**256 - P))
        elif sub == 1:
            put(S, i, N + (int(i) * 2654435761 * 2**64) % (2**256 - N))
        elif sub == 2:
            put(R, i, bad_x[(i // 32) % 64])
        else:
            rr = (one(R, i) * 3 + 1) % P
            put(R, i, rr)
            put(S, i, model.challenge(rr, one(PX, i), M[i].tobytes()) * dprime(i) % N)
    PXd, Rd, Sd = (engine.to_device(a) for a in (PX, R, S))
    Md = torch.from_numpy(M).to(engine.tdev)
    got = engine.to_numpy(engine.schnorr_verify(PXd, Md, Rd, Sd))
    want = model.chain_of_existing_calls(engine, PXd, Md, Rd, Sd)
    assert np.array_equal(got, want), np.nonzero(got != want)[0][:10]
    assert np.array_equal(got, (cls <= 2).astype(np.uint8)), np.nonzero(got != (cls <= 2))[0][:10]      # three classes in eight are accepted, five refused
    for i in list(range(0, 64)) + list(range(n - 16, n)):          # and a sample against the model
        assert bool(got[i]) == model.verify(one(PX, i), M[i].tobytes(), one(R, i), one(S, i)), i


# ---------------------------------------------------------------- 5. round trip across the chunk edge
def test_round_trip_across_the_chunk_boundary_by_three(engine):
    import torch
    n = CHUNK + 3
    g = torch.Generator(device="cpu"); g.manual_seed(341)
    D = torch.randint(-2**63, 2**63 - 1, (n, 4), dtype=torch.int64, generator=g)
    D[:, 3] &= 0x3fffffffffffffff
    D = D.to(engine.tdev)
    A = torch.randint(-2**63, 2**63 - 1, (n, 4), dtype=torch.int64, generator=g).to(engine.tdev)
    msgs = torch.randint(0, 256, (n, 32), dtype=torch.uint8, generator=g).to(engine.tdev)
    px, r, s, ok = engine.schnorr_sign(D, msgs, aux=A)
    assert bool(ok.all())
    assert bool(engine.schnorr_verify(px, msgs, r, s).all())
    rows = sorted(set(list(range(0, n, n // 1024))[:1024] + [CHUNK - 2, CHUNK - 1, CHUNK, CHUNK + 1, CHUNK + 2, n - 1]))      # a strided sample and the edge
    assert len(rows) >= 1024
    sel = lambda t: ints(engine, engine.select_rows(t, rows))
    d_i, a_i, m_i = sel(D), sel(A), msgs.cpu().numpy()[rows]
    got = list(zip(sel(px), sel(r), sel(s)))
    assert got == [model.sign(d_i[j], m_i[j].tobytes(), a_i[j]) for j in range(len(rows))]


# ---------------------------------------------------------------- 6. refusals
def test_keys_out_of_range_are_refused_lane_by_lane(engine):
    import torch
    d = [5, 0, 6, N, 7, N + 1, 8, 2**256 - 1, 9, N - 1, 1]
    rows = np.random.default_rng(6).integers(0, 256, size=(len(d), 32), dtype=np.uint8)
    px, r, s, ok = engine.schnorr_sign(up(engine, d), torch.from_numpy(rows).to(engine.tdev), aux=up(engine, list(range(len(d)))))
    want = [model.sign(a, rows[i].tobytes(), i) for i, a in enumerate(d)]
    assert [w is None for w in want] == [not 1 <= a < N for a in d]
    assert flags(engine, ok) == [0 if w is None else 1 for w in want]
    assert list(zip(ints(engine, px), ints(engine, r), ints(engine, s))) == [(0, 0, 0) if w is None else w for w in want]


def test_bad_arguments_are_refused(engine):
    import ctypes as C
    import torch
    from ecsimd_amd.engine import EcsimdHipError
    empty, none = engine.empty(0), torch.zeros((0, 32), dtype=torch.uint8, device=engine.tdev)
    assert engine.schnorr_sign(empty, none)[1].shape[0] == 0 and engine.schnorr_verify(empty, none, empty, empty).shape[0] == 0      # n = 0
    d = up(engine, [5, 6]); msgs = torch.zeros((2, 32), dtype=torch.uint8, device=engine.tdev); out = [engine.empty(2) for _ in range(3)]; ok = engine.flags(2)
    lib, ctx = engine.lib, engine.ctx
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)
    sign = lambda dd, m, stride, aux, px, r, s, okk, n=2: lib.ecsimd_hip_schnorr_sign(ctx, p(dd), p(m), C.c_size_t(32), C.c_size_t(stride), p(aux), p(px), p(r), p(s), p(okk), C.c_size_t(n))
    verify = lambda px, m, stride, r, s, okk, n=2: lib.ecsimd_hip_schnorr_verify(ctx, p(px), p(m), C.c_size_t(32), C.c_size_t(stride), p(r), p(s), p(okk), C.c_size_t(n))
    BAD = -1
    assert sign(d, msgs, 32, None, out[0], out[1], out[2], ok) == 0
    for args in ((None, msgs, 32, None, out[0], out[1], out[2], ok), (d, None, 32, None, out[0], out[1], out[2], ok), (d, msgs, 32, None, out[0], None, out[2], ok),
                 (d, msgs, 32, None, out[0], out[1], None, ok), (d, msgs, 32, None, out[0], out[1], out[2], None)):                    # null pointers
        assert sign(*args) == BAD
    for args in ((d, msgs, 32, None, out[0], d, out[2], ok), (d, msgs, 32, None, out[0], out[1], out[1], ok), (d, msgs, 32, None, out[1], out[1], out[2], ok),
                 (d, msgs, 32, out[2], out[0], out[1], out[2], ok), (d, msgs, 32, None, d, out[1], out[2], ok)):                        # aliased outputs
        assert sign(*args) == BAD
        assert b"alias" in lib.ecsimd_hip_last_error(ctx)
    assert sign(d, msgs, 31, None, out[0], out[1], out[2], ok) == BAD and b"stride" in lib.ecsimd_hip_last_error(ctx)                  # stride < msg_bytes
    assert verify(out[0], msgs, 32, out[1], out[2], ok) == 0
    for args in ((None, msgs, 32, out[1], out[2], ok), (out[0], None, 32, out[1], out[2], ok), (out[0], msgs, 32, None, out[2], ok),
                 (out[0], msgs, 32, out[1], None, ok), (out[0], msgs, 32, out[1], out[2], None), (out[0], msgs, 31, out[1], out[2], ok)):
        assert verify(*args) == BAD
    # a context that squares like the reference has no such algorithm
    engine.set_ref_square_compat(True)
    try:
        for call in (lambda: engine.schnorr_sign(d, msgs), lambda: engine.schnorr_verify(out[0], msgs, out[1], out[2])):
            with pytest.raises(EcsimdHipError, match="REF_SQUARE_COMPAT"):
                call()
        assert sign(d, msgs, 32, None, out[0], out[1], out[2], ok) == BAD
    finally:
        engine.set_ref_square_compat(False)
    assert sign(d, msgs, 32, None, out[0], out[1], out[2], ok) == 0
    with pytest.raises(EcsimdHipError):                             # operands of different length
        engine.schnorr_sign(up(engine, [5]), msgs)


# ---------------------------------------------------------------- 7. what the workspace holds afterwards
def test_the_workspace_is_zero_after_signing(engine):
    import torch
    n = 3000
    d = random_keys(np.random.default_rng(7), n)
    msgs = torch.randint(0, 256, (n, 32), dtype=torch.uint8).to(engine.tdev)
    px, r, s, ok = engine.schnorr_sign(up(engine, d), msgs, aux=up(engine, d[::-1]))
    assert all(flags(engine, ok))
    ws = engine.workspace_bytes()
    assert ws.size >= n * 256 and not ws[:n * 256].any()           # the Jacobian product, d G, k0 G, k0: 8 x 32 B per element, all of it
