"""GPU suite: BIP-340 batch verification on the device (include/ecsimd_schnorr_batch.h): Engine.schnorr_verify_batch on both routes and
Engine.schnorr_batch_randomizers.

The signatures are made on the device by Engine.schnorr_sign, so the expected verdict is known by construction; every test cross-checks it against the AND of
Engine.schnorr_verify over the same operands.  The randomizers are compared bit for bit with tools/schnorr_batch_model.py (hashlib).  Sizes are the edges of
the fan-16 trees up to four levels."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

from helpers import ints_to_arr, arr_to_ints

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bip340_model as b340            # noqa: E402
import schnorr_batch_model as model    # noqa: E402

pytestmark = pytest.mark.gpu
P, N = b340.P, b340.N
AUTO, MSM, LANES = 0, 1, 2
SIZES = (1, 2, 15, 16, 17, 255, 256, 257, 4097)
LENGTHS = (0, 32, 33, 100)
TOTAL = 4100                          # lanes signed per message length: the largest size and a few spare ones to borrow an r from
BAD_ARG = -1


def up(engine, ints):
    return engine.to_device(ints_to_arr([int(x) for x in ints]) if len(ints) else np.zeros((0, 4), dtype=np.uint64))


def ints(engine, t):
    return arr_to_ints(engine.to_numpy(t))


def non_curve_x(seed):
    rng = np.random.default_rng(seed)
    while True:
        x = int.from_bytes(rng.bytes(32), "big") % P
        if b340.lift_x(x) is None:
            return x


_SIGNED = {}


def signed(engine, length):
    """TOTAL valid signatures over messages of `length` bytes: device tensors and the same values as Python integers / bytes.  Lane 0 has d = 1 (P = G: the key
    sum meets G twice), lane 1 d = n - 1.  Made once per length and never changed: the tests work on copies."""
    import torch
    if length not in _SIGNED:
        rng = np.random.default_rng(1000 + length)
        d = [1, N - 1] + [int.from_bytes(rng.bytes(32), "big") % (N - 1) + 1 for _ in range(TOTAL - 2)]
        rows = rng.integers(0, 256, size=(TOTAL, length), dtype=np.uint8)
        msgs = torch.from_numpy(rows).to(engine.tdev)
        aux = up(engine, [int.from_bytes(rng.bytes(32), "big") for _ in range(TOTAL)])
        px, r, s, ok = engine.schnorr_sign(up(engine, d), msgs, aux=aux)
        assert engine.to_numpy(ok).all()
        assert engine.to_numpy(engine.schnorr_verify(px, msgs, r, s)).all()
        _SIGNED[length] = dict(px=px, r=r, s=s, msgs=msgs, ipx=ints(engine, px), ir=ints(engine, r), i_s=ints(engine, s), rows=[bytes(row) for row in rows])
    return _SIGNED[length]


def take(engine, S, u):
    """The first u lanes as fresh device tensors and as host lists."""
    return dict(px=S["px"][:u].clone(), r=S["r"][:u].clone(), s=S["s"][:u].clone(), msgs=S["msgs"][:u].clone(),
                ipx=list(S["ipx"][:u]), ir=list(S["ir"][:u]), i_s=list(S["i_s"][:u]), rows=list(S["rows"][:u]))


def set_lane(engine, B, what, lane, value):
    """One lane of px, r, s (an integer) or msgs (bytes) replaced on the device and in the host copy."""
    import torch
    if what == "msgs":
        B["msgs"][lane] = torch.from_numpy(np.frombuffer(value, dtype=np.uint8).copy()).to(engine.tdev)
        B["rows"][lane] = value
    else:
        B[what][lane] = up(engine, [value])[0]
        B[{"px": "ipx", "r": "ir", "s": "i_s"}[what]][lane] = value


def verdict(engine, B, route):
    """ok[0] of one call, with ok preset to 0xAA."""
    import torch
    ok = torch.full((1,), 0xAA, dtype=torch.uint8, device=engine.tdev)
    got = engine.schnorr_verify_batch(B["px"], B["msgs"], B["r"], B["s"], route=route, out=ok)
    assert got is ok
    v = int(ok.cpu()[0])
    assert v in (0, 1), v
    return v


def lane_by_lane(engine, B):
    """The AND of Engine.schnorr_verify: what every route has to agree with."""
    return int(bool(engine.to_numpy(engine.schnorr_verify(B["px"], B["msgs"], B["r"], B["s"])).all()))


def device_randomizers(engine, B):
    a = ints(engine, engine.schnorr_batch_randomizers(B["px"], B["msgs"], B["r"], B["s"]))
    return [int(x) for x in a]


def model_randomizers(B):
    return model.randomizers(B["ipx"], B["rows"], B["ir"], B["i_s"])


# ---------------------------------------------------------------- 1. the randomizers, bit for bit
@pytest.mark.parametrize("length", LENGTHS)
def test_randomizers_are_the_models_at_every_tree_shape(engine, length):
    S = signed(engine, length)
    for u in SIZES:
        B = take(engine, S, u)
        a = device_randomizers(engine, B)
        assert a == model_randomizers(B), (u, length)
        assert all(x & 1 and x < 1 << 128 for x in a), (u, length)
        assert a == device_randomizers(engine, B), (u, length)               # the same batch, the same randomizers: nothing is drawn
    assert ints(engine, engine.schnorr_batch_randomizers(*(S[k][:0] for k in ("px", "msgs", "r", "s")))) == []


@pytest.mark.parametrize("u", (17, 257, 4097))
def test_one_flipped_bit_anywhere_changes_every_randomizer(engine, u):
    S = signed(engine, 32)
    base = take(engine, S, u)
    a0 = device_randomizers(engine, base)
    lane = u // 2
    for what, value in (("msgs", bytes([S["rows"][lane][0] ^ 0x20]) + S["rows"][lane][1:]), ("s", S["i_s"][lane] ^ (1 << 200)),
                        ("r", S["ir"][lane] ^ 1), ("px", S["ipx"][lane] ^ (1 << 255))):
        B = take(engine, S, u)
        set_lane(engine, B, what, lane, value)
        a = device_randomizers(engine, B)
        assert a == model_randomizers(B), what                                # malformed lanes included: their bytes are hashed as they are
        assert all(x != y for x, y in zip(a, a0)), what


# ---------------------------------------------------------------- 2. acceptance
@pytest.mark.parametrize("u", SIZES)
def test_valid_batches_are_accepted_on_every_route(engine, u):
    for length in ((32,) if u > 257 else (32, 33)):
        B = take(engine, signed(engine, length), u)
        assert lane_by_lane(engine, B) == 1
        for route in (MSM, LANES, AUTO):
            assert verdict(engine, B, route) == 1, (u, length, route)
            assert verdict(engine, B, route) == 1, (u, length, route, "again")      # the workspace of the first call is the second one's


def test_equal_lanes_and_the_empty_batch_are_accepted(engine):
    S = signed(engine, 32)
    u = 257
    B = dict(px=S["px"][5:6].repeat(u, 1).contiguous(), r=S["r"][5:6].repeat(u, 1).contiguous(), s=S["s"][5:6].repeat(u, 1).contiguous(),
             msgs=S["msgs"][5:6].repeat(u, 1).contiguous())
    assert lane_by_lane(engine, B) == 1
    for route in (MSM, LANES):
        assert verdict(engine, B, route) == 1, route
    empty = dict(px=S["px"][:0], r=S["r"][:0], s=S["s"][:0], msgs=S["msgs"][:0])
    for route in (MSM, LANES, AUTO):
        assert verdict(engine, empty, route) == 1, route


# ---------------------------------------------------------------- 3. refusal
def corruptions(S, lane):
    """(name, operand, value) for lane `lane`: one changed operand each, every one of them an invalid signature."""
    other = (lane + 1) % TOTAL if lane != 0 else 2          # (lanes 0 and 1 share their x-only key; their r differ anyway)
    return [
        ("a bit of s", "s", S["i_s"][lane] ^ (1 << 77)),
        ("s = n", "s", N),
        ("s = 2^256 - 1", "s", (1 << 256) - 1),
        ("another lane's r", "r", S["ir"][other]),
        ("r on no point", "r", non_curve_x(lane)),
        ("r = p + 1", "r", P + 1),                           # x = 1 is on the curve: refused for its range
        ("px on no point", "px", non_curve_x(lane + 7)),
        ("px = p + 1", "px", P + 1),
        ("a message bit", "msgs", S["rows"][lane][:31] + bytes([S["rows"][lane][31] ^ 0x80])),
    ]


@pytest.mark.parametrize("u", (1, 17, 257, 4097))
def test_one_corrupted_lane_refuses_the_batch_on_both_routes(engine, u):
    S = signed(engine, 32)
    assert b340.lift_x(1) is not None and P + 1 < 1 << 256
    for lane in sorted({0, u // 2, u - 1}):
        for name, what, value in corruptions(S, lane):
            B = take(engine, S, u)
            set_lane(engine, B, what, lane, value)
            assert lane_by_lane(engine, B) == 0, (u, lane, name)
            for route in (MSM, LANES):
                assert verdict(engine, B, route) == 0, (u, lane, name, route)
    B = take(engine, S, u)                                                       # and the untouched batch is still accepted afterwards
    assert verdict(engine, B, MSM) == 1 and verdict(engine, B, LANES) == 1


@pytest.mark.parametrize("u", (2, 17, 257))
def test_errors_that_cancel_without_randomizers_are_refused(engine, u):
    S = signed(engine, 32)
    delta = 0x1F2E3D4C5B6A79
    i, j = 0, u - 1
    B = take(engine, S, u)
    set_lane(engine, B, "s", i, (S["i_s"][i] + delta) % N)
    set_lane(engine, B, "s", j, (S["i_s"][j] - delta) % N)
    assert sum(B["i_s"]) % N == sum(S["i_s"][:u]) % N                          # the unweighted sum of the s is what it was
    assert lane_by_lane(engine, B) == 0
    for route in (MSM, LANES):
        assert verdict(engine, B, route) == 0, route
    # lanes i and j exact copies of one signature: their errors cancel unless the lane index enters a_i
    B = take(engine, S, u)
    for what, src in (("px", "ipx"), ("r", "ir"), ("s", "i_s"), ("msgs", "rows")):
        set_lane(engine, B, what, i, S[src][3]); set_lane(engine, B, what, j, S[src][3])
    assert lane_by_lane(engine, B) == 1 and verdict(engine, B, MSM) == 1
    a = device_randomizers(engine, B)
    assert a[i] != a[j]
    set_lane(engine, B, "s", i, (S["i_s"][3] + delta) % N)
    set_lane(engine, B, "s", j, (S["i_s"][3] - delta) % N)
    assert lane_by_lane(engine, B) == 0
    for route in (MSM, LANES):
        assert verdict(engine, B, route) == 0, route


# ---------------------------------------------------------------- 4. the BIP's vectors
def test_the_bips_vectors_by_message_length(engine):
    """tests/golden/bip340_vectors.json, grouped by message length: the valid vectors of a length pass together; with any one invalid vector of that length
    added the batch is refused.  A vector counts as invalid where the file says so (`verification_result`) -- and, as the file may hold valid ones only, each
    valid vector is also turned into the BIP's kinds of invalid ones: s negated, s = n, r = p, the key off the curve, another message."""
    import torch
    kat = json.load(open(os.path.join(ROOT, "tests", "golden", "bip340_vectors.json")))
    groups = {}
    for c in kat["cases"]:
        sig, msg = bytes.fromhex(c["signature"]), bytes.fromhex(c["message"])
        v = dict(ipx=int(c["public_key"], 16), ir=int.from_bytes(sig[:32], "big"), i_s=int.from_bytes(sig[32:], "big"), row=msg,
                 valid=str(c.get("verification_result", "TRUE")).upper() == "TRUE")
        assert b340.verify(v["ipx"], msg, v["ir"], v["i_s"]) == v["valid"]
        groups.setdefault(len(msg), []).append(v)

    def batch_of(vs):
        rows = np.frombuffer(b"".join(v["row"] for v in vs), dtype=np.uint8).reshape(len(vs), len(vs[0]["row"])).copy()
        return dict(px=up(engine, [v["ipx"] for v in vs]), r=up(engine, [v["ir"] for v in vs]), s=up(engine, [v["i_s"] for v in vs]),
                    msgs=torch.from_numpy(rows).to(engine.tdev))

    assert groups
    for length, vs in groups.items():
        good = [v for v in vs if v["valid"]]
        assert good
        derived = []
        for v in good:
            derived += [dict(v, i_s=N - v["i_s"]), dict(v, i_s=N), dict(v, ir=P), dict(v, ipx=non_curve_x(length)),
                        dict(v, row=bytes([v["row"][0] ^ 1]) + v["row"][1:]) if length else dict(v, ir=v["ir"] ^ 2)]
        B = batch_of(good)
        assert lane_by_lane(engine, B) == 1
        for route in (MSM, LANES, AUTO):
            assert verdict(engine, B, route) == 1, (length, route)
        for bad in [v for v in vs if not v["valid"]] + derived:
            assert not b340.verify(bad["ipx"], bad["row"], bad["ir"], bad["i_s"])
            for at in (0, len(good)):
                B = batch_of(good[:at] + [bad] + good[at:])
                assert lane_by_lane(engine, B) == 0
                for route in (MSM, LANES):
                    assert verdict(engine, B, route) == 0, (length, route, at)


# ---------------------------------------------------------------- 5. arguments
def test_bad_arguments_are_refused_with_a_message_and_ok_is_untouched(engine):
    import torch
    from ecsimd_amd import Engine
    S = signed(engine, 32)
    u = 17
    B = take(engine, S, u)
    eng = Engine(0)
    try:
        lib = eng.lib
        ok = torch.full((16,), 0xAA, dtype=torch.uint8, device=eng.tdev)
        a = eng.empty(u)
        torch.cuda.synchronize()
        eng._bind_stream()
        ptr = lambda t, off=0: C.c_void_p(t.data_ptr() + off)

        def verify(px=ptr(B["px"]), msg=ptr(B["msgs"]), r=ptr(B["r"]), s=ptr(B["s"]), okp=ptr(ok), n=u, flags=MSM, length=32, stride=32):
            rc = lib.ecsimd_schnorr_verify_batch(eng.ctx, px, msg, C.c_size_t(length), C.c_size_t(stride), r, s, okp, C.c_size_t(n), C.c_int(flags))
            return rc, lib.ecsimd_hip_last_error(eng.ctx).decode()

        def randomizers(px=ptr(B["px"]), msg=ptr(B["msgs"]), r=ptr(B["r"]), s=ptr(B["s"]), ap=ptr(a), n=u):
            rc = lib.ecsimd_schnorr_batch_randomizers(eng.ctx, px, msg, C.c_size_t(32), C.c_size_t(32), r, s, ap, C.c_size_t(n))
            return rc, lib.ecsimd_hip_last_error(eng.ctx).decode()

        null = C.c_void_p(0)
        cases = {
            "flag 3": verify(flags=3), "flag 4": verify(flags=4), "flag -1": verify(flags=-1),
            "px null": verify(px=null), "r null": verify(r=null), "s null": verify(s=null), "msg null": verify(msg=null), "ok null": verify(okp=null),
            "px misaligned": verify(px=ptr(B["px"], 8)), "r misaligned": verify(r=ptr(B["r"], 8)), "s misaligned": verify(s=ptr(B["s"], 4)),
            "stride below the length": verify(stride=31),
            "ok inside px": verify(okp=ptr(B["px"], 5)), "ok inside r": verify(okp=ptr(B["r"], 32 * u - 1)), "ok inside s": verify(okp=ptr(B["s"])),
            "ok inside msg": verify(okp=ptr(B["msgs"], 32 * u - 1)),
            "n too large": verify(n=(1 << 24)), "n far too large": verify(n=(1 << 40)),
            "a null": randomizers(ap=null), "a misaligned": randomizers(ap=ptr(a, 8)), "a is r": randomizers(ap=ptr(B["r"])),
            "a inside s": randomizers(ap=ptr(B["s"], 32 * (u - 1))), "a inside px": randomizers(ap=ptr(B["px"], 16)), "randomizers: n too large": randomizers(n=1 << 24),
            "randomizers: px null": randomizers(px=null),
        }
        for name, (rc, said) in cases.items():
            assert rc == BAD_ARG and said.startswith("bad argument: ") and len(said) > 20, (name, rc, said)
        assert "overlap" in cases["ok inside r"][1] and "overlap" in cases["a is r"][1] and "MAX_N" in cases["n too large"][1] and "flags" in cases["flag 3"][1]
        torch.cuda.synchronize()
        assert bytes(ok.cpu().numpy()) == b"\xaa" * 16
        eng.set_ref_square_compat(True)
        for rc, said in (verify(flags=LANES), verify(flags=MSM), randomizers()):
            assert rc == BAD_ARG and "REF_SQUARE_COMPAT" in said, said
        eng.set_ref_square_compat(False)
        torch.cuda.synchronize()
        assert bytes(ok.cpu().numpy()) == b"\xaa" * 16
        assert verify()[0] == 0 and verify(flags=LANES, okp=ptr(ok, 1))[0] == 0 and randomizers()[0] == 0
        torch.cuda.synchronize()
        assert bytes(ok.cpu().numpy()) == b"\x01\x01" + b"\xaa" * 14
        assert [int(x) for x in ints(eng, a)] == model_randomizers(B)
    finally:
        eng.close()


# ---------------------------------------------------------------- 6. stream capture
def captured(fn):
    import torch
    side = torch.cuda.Stream(); side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            out = fn()
    torch.cuda.synchronize()                                             # the capture ended without error
    return g, out


def test_a_captured_call_replays_the_verdict_of_what_is_in_the_buffers(engine):
    import torch
    from ecsimd_amd import Engine
    u = 257
    B = take(engine, signed(engine, 32), u)
    torch.cuda.synchronize()
    eng = Engine(0)
    try:
        oks = {route: torch.full((1,), 0xAA, dtype=torch.uint8, device=eng.tdev) for route in (MSM, LANES)}
        for route in (MSM, LANES):                                       # the warm-up at the capture's (n, msg_bytes, flags)
            eng.schnorr_verify_batch(B["px"], B["msgs"], B["r"], B["s"], route=route, out=oks[route])
        torch.cuda.synchronize()
        for route in (MSM, LANES):
            oks[route].fill_(0xAA)
            g, _ = captured(lambda: eng.schnorr_verify_batch(B["px"], B["msgs"], B["r"], B["s"], route=route, out=oks[route]))
            g.replay(); torch.cuda.synchronize()
            assert int(oks[route].cpu()[0]) == 1, route
            good = B["s"][100].clone()
            B["s"][100] = up(eng, [(ints(eng, good.reshape(1, 4))[0] + 1) % N])[0]      # one s overwritten in place
            torch.cuda.synchronize()
            g.replay(); torch.cuda.synchronize()
            assert int(oks[route].cpu()[0]) == 0, route
            B["s"][100] = good
            torch.cuda.synchronize()
            g.replay(); torch.cuda.synchronize()
            assert int(oks[route].cpu()[0]) == 1, route
            del g
    finally:
        eng.close()


def test_a_capture_without_a_warm_up_is_refused_and_stays_valid(engine):
    import torch
    from ecsimd_amd import Engine, EcsimdHipError
    u = 257
    B = take(engine, signed(engine, 32), u)
    torch.cuda.synchronize()
    eng = Engine(0)
    try:
        ok = torch.full((1,), 0xAA, dtype=torch.uint8, device=eng.tdev)
        mark = torch.zeros((4,), dtype=torch.uint8, device=eng.tdev)
        said = {}

        def body():
            for route in (MSM, LANES):
                try:
                    eng.schnorr_verify_batch(B["px"], B["msgs"], B["r"], B["s"], route=route, out=ok)
                except EcsimdHipError as exc:
                    said[route] = str(exc)
            try:
                eng.schnorr_batch_randomizers(B["px"], B["msgs"], B["r"], B["s"])
            except EcsimdHipError as exc:
                said["a"] = str(exc)
            mark.add_(1)                                                 # something the capture does hold
        g, _ = captured(body)
        assert sorted(map(str, said)) == ["1", "2", "a"] and all("capture" in msg and "(-1)" in msg for msg in said.values()), said
        g.replay(); torch.cuda.synchronize()
        assert int(ok.cpu()[0]) == 0xAA and mark.cpu().tolist() == [1, 1, 1, 1]
        del g
        for route in (MSM, LANES):                                       # outside a capture the same context runs the call
            assert int(eng.schnorr_verify_batch(B["px"], B["msgs"], B["r"], B["s"], route=route).cpu()[0]) == 1
    finally:
        eng.close()
