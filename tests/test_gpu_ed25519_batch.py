"""GPU suite: Ed25519 batch verification on the device (include/ecsimd_ed25519_batch.h): Engine.ed25519_verify_batch on both routes,
Engine.ed25519_verify_cofactored, Engine.ed25519_batch_randomizers.

Honest signatures are made on the device by Engine.ed25519_sign, so their verdict is known by construction; the refused, small-order and mixed-order lanes are
tests/golden/ed25519_verdicts.json's, with the verdict of tools/ed25519_batch_model.py's cofactored rule computed once for the whole file.  Every batch verdict
is cross-checked against the AND of Engine.ed25519_verify_cofactored over the same operands; the randomizers are compared bit for bit with the model."""
import ctypes as C
import functools
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import ed25519_model as ed             # noqa: E402
import ed25519_batch_model as model    # noqa: E402

pytestmark = pytest.mark.gpu
L, P = ed.L, ed.P
SMALL, AUTO, MSM, LANES = 1, 0, 2, 4
ROUTES = (MSM, LANES)
SIZES = (0, 1, 2, 16, 17, 257)
LENGTHS = (0, 1, 111, 112, 300)
TOTAL = 260
BAD_ARG = -1


def le32(v):
    return int(v).to_bytes(32, "little")


def dev_rows(engine, rows, width, offset=None):
    """A list of byte strings of `width` bytes -> an (n, width) uint8 device tensor; offset: a view that many bytes into a larger allocation."""
    import torch
    n = len(rows)
    a = np.frombuffer(b"".join(rows), dtype=np.uint8).reshape(n, width).copy() if n and width else np.zeros((n, width), dtype=np.uint8)
    t = torch.from_numpy(a).to(engine.tdev)
    if offset is None:
        return t
    buf = torch.zeros(width * n + 8, dtype=torch.uint8, device=engine.tdev)
    view = buf[offset:offset + width * n].view(n, width)
    view.copy_(t)
    assert view.data_ptr() % 4 == offset % 4
    return view


class Batch:
    """pk, msg, sig per lane on the host; tensors made on demand.  Messages of one length travel without lens, others in rows of the longest with lens."""
    def __init__(self, pks, msgs, sigs):
        self.pks, self.msgs, self.sigs = list(pks), list(msgs), list(sigs)

    def __len__(self):
        return len(self.pks)

    def copy(self):
        return Batch(self.pks, self.msgs, self.sigs)

    def tensors(self, engine, offset=None, stride=None):
        import torch
        n = len(self)
        lengths = {len(m) for m in self.msgs}
        width = max(lengths) if lengths else 0
        lens = None
        if len(lengths) > 1 or (stride is not None and stride != width):
            width = max(width, stride or 0)
            lens = torch.tensor([len(m) for m in self.msgs], dtype=torch.int32, device=engine.tdev)
        rows = [m + bytes(width - len(m)) for m in self.msgs]
        return dev_rows(engine, self.pks, 32, offset), dev_rows(engine, rows, width, offset), dev_rows(engine, self.sigs, 64, offset), lens

    def model_randomizers(self):
        return model.randomizers(self.pks, self.msgs, self.sigs)


def verdict(engine, B, flags, **how):
    """ok[0] of one call, with ok preset to 0xAA."""
    import torch
    pk, msgs, sig, lens = B.tensors(engine, **how)
    ok = torch.full((1,), 0xAA, dtype=torch.uint8, device=engine.tdev)
    got = engine.ed25519_verify_batch(pk, msgs, sig, lens=lens, flags=flags, out=ok)
    assert got is ok
    v = int(ok.cpu()[0])
    assert v in (0, 1), v
    return v


def per_lane(engine, B, small=False, **how):
    pk, msgs, sig, lens = B.tensors(engine, **how)
    return engine.ed25519_verify_cofactored(pk, msgs, sig, lens=lens, reject_small_order=small).cpu().tolist()


def both_routes(engine, B, want, small=False, **how):
    """Every route's verdict is `want`, and so is the AND of the per-lane rule."""
    lanes = per_lane(engine, B, small, **how)
    assert int(all(lanes)) == want, lanes
    for route in ROUTES:
        assert verdict(engine, B, route | (SMALL if small else 0), **how) == want, (route, small, how)
    return lanes


def device_randomizers(engine, B, **how):
    pk, msgs, sig, lens = B.tensors(engine, **how)
    z = engine.ed25519_batch_randomizers(pk, msgs, sig, lens=lens).cpu().numpy()
    return [int.from_bytes(bytes(r), "little") for r in z]


_SIGNED = {}


def signed(engine, length):
    """TOTAL honest signatures over messages of `length` bytes, made on the device once per length and never changed (the tests work on copies)."""
    import torch
    if length not in _SIGNED:
        rng = np.random.default_rng(2000 + length)
        seeds = torch.from_numpy(rng.integers(0, 256, size=(TOTAL, 32), dtype=np.uint8)).to(engine.tdev)
        rows = rng.integers(0, 256, size=(TOTAL, length), dtype=np.uint8)
        msgs = torch.from_numpy(rows).to(engine.tdev)
        sig, pk = engine.ed25519_sign(seeds, msgs)
        assert engine.ed25519_verify(pk, msgs, sig).cpu().tolist() == [1] * TOTAL
        _SIGNED[length] = Batch([bytes(r) for r in pk.cpu().numpy()], [bytes(r) for r in rows], [bytes(r) for r in sig.cpu().numpy()])
    return _SIGNED[length]


def take(B, n, first=0):
    return Batch(B.pks[first:first + n], B.msgs[first:first + n], B.sigs[first:first + n])


@functools.lru_cache(maxsize=None)
def records():
    """The verdict fixture with the model's cofactored verdicts (computed once: a few seconds of host time)."""
    out = []
    for r in json.load(open(os.path.join(ROOT, "tests", "golden", "ed25519_verdicts.json")))["records"]:
        pk, msg, sig = bytes.fromhex(r["public_key"]), bytes.fromhex(r["message"]), bytes.fromhex(r["signature"])
        out.append(dict(kind=r["kind"], pk=pk, msg=msg, sig=sig, plain=r["model"], cof=int(model.verify_cofactored(pk, msg, sig)),
                        cof_strict=int(model.verify_cofactored(pk, msg, sig, True))))
    return tuple(out)


def batch_of(lanes):
    return Batch([x["pk"] for x in lanes], [x["msg"] for x in lanes], [x["sig"] for x in lanes])


# ---------------------------------------------------------------- 1. sizes, message lengths, lens, alignment
@pytest.mark.parametrize("length", LENGTHS)
def test_valid_batches_of_every_size_are_accepted_and_the_randomizers_are_the_models(engine, length):
    S = signed(engine, length)
    for n in SIZES:
        B = take(S, n)
        assert both_routes(engine, B, 1) == [1] * n, (n, length)
        assert verdict(engine, B, AUTO) == 1 and verdict(engine, B, MSM | SMALL) == 1, (n, length)
        z = device_randomizers(engine, B)
        assert z == B.model_randomizers(), (n, length)
        assert all(x & 1 and x < 1 << 128 for x in z)
    assert verdict(engine, take(S, 17), MSM) == 1                        # the workspace of a larger batch serves a smaller one


def test_per_lane_lengths(engine):
    rng = np.random.default_rng(5)
    S = signed(engine, 300)
    n = 257
    cut = [int(v) for v in rng.integers(0, 301, size=n)]
    cut[:6] = [0, 1, 111, 112, 300, 299]
    # a signature over a prefix is another message: sign the prefixes on the device through lens
    import torch
    seeds = torch.from_numpy(rng.integers(0, 256, size=(n, 32), dtype=np.uint8)).to(engine.tdev)
    rows = dev_rows(engine, S.msgs[:n], 300)
    lens = torch.tensor(cut, dtype=torch.int32, device=engine.tdev)
    sig, pk = engine.ed25519_sign(seeds, rows, lens=lens)
    B = Batch([bytes(r) for r in pk.cpu().numpy()], [m[:c] for m, c in zip(S.msgs, cut)], [bytes(r) for r in sig.cpu().numpy()])
    for how in (dict(stride=300), dict(stride=301, offset=1)):
        assert both_routes(engine, B, 1, **how) == [1] * n
        assert device_randomizers(engine, B, **how) == B.model_randomizers()
    # one lane a byte shorter or longer than what was signed
    for lane, d in ((2, -1), (3, 1), (n - 1, 1 if cut[n - 1] < 300 else -1)):
        B2 = B.copy()
        B2.msgs[lane] = S.msgs[lane][:cut[lane] + d]
        lanes = both_routes(engine, B2, 0, stride=300)
        assert lanes == [int(i != lane) for i in range(n)]


@pytest.mark.parametrize("offset", (1, 2, 3))
def test_unaligned_bases(engine, offset):
    for length in (1, 111, 112):
        B = take(signed(engine, length), 17)
        assert both_routes(engine, B, 1, offset=offset) == [1] * 17
        assert device_randomizers(engine, B, offset=offset) == B.model_randomizers()
        B.sigs[16] = B.sigs[16][:32] + le32(int.from_bytes(B.sigs[16][32:], "little") ^ 2)
        assert both_routes(engine, B, 0, offset=offset) == [1] * 16 + [0]


# ---------------------------------------------------------------- 2. forgeries
def forged(S, B, lane, kind):
    pk, msg, sig = B.pks[lane], B.msgs[lane], B.sigs[lane]
    if kind == "flipped s":
        B.sigs[lane] = sig[:32] + le32(int.from_bytes(sig[32:], "little") ^ (1 << 77))
    elif kind == "flipped message":
        B.msgs[lane] = bytes([msg[0] ^ 0x10]) + msg[1:]
    elif kind == "another key":
        B.pks[lane] = S.pks[TOTAL - 1 - lane]
    return B


@pytest.mark.parametrize("n", (17, 257))
def test_one_forged_lane_refuses_the_batch(engine, n):
    S = signed(engine, 112)
    for lane in (0, 16, n - 1):
        for kind in ("flipped s", "flipped message", "another key"):
            B = forged(S, take(S, n), lane, kind)
            assert both_routes(engine, B, 0) == [int(i != lane) for i in range(n)], (lane, kind)
    assert both_routes(engine, take(S, n), 1) == [1] * n                  # and the untouched batch is still accepted afterwards


@pytest.mark.parametrize("n", (2, 17, 257))
def test_forgeries_that_cancel_under_unit_weights_are_refused(engine, n):
    S = signed(engine, 111)
    B = take(S, n)
    i, j = 0, n - 1
    B.sigs[i] = B.sigs[i][:32] + le32((int.from_bytes(B.sigs[i][32:], "little") + 1) % L)
    B.sigs[j] = B.sigs[j][:32] + le32((int.from_bytes(B.sigs[j][32:], "little") - 1) % L)
    assert sum(int.from_bytes(s[32:], "little") for s in B.sigs) % L == sum(int.from_bytes(s[32:], "little") for s in S.sigs[:n]) % L
    assert both_routes(engine, B, 0) == [0] + [1] * (n - 2) + [0]
    # lanes i and j exact copies of one signature: only the lane index tells their randomizers apart
    B = take(S, n)
    for lane in (i, j):
        B.pks[lane], B.msgs[lane], B.sigs[lane] = S.pks[3], S.msgs[3], S.sigs[3]
    assert both_routes(engine, B, 1) == [1] * n
    z = device_randomizers(engine, B)
    assert z[i] != z[j]
    s3 = int.from_bytes(S.sigs[3][32:], "little")
    B.sigs[i] = S.sigs[3][:32] + le32((s3 + 1) % L); B.sigs[j] = S.sigs[3][:32] + le32((s3 - 1) % L)
    assert both_routes(engine, B, 0) == [0] + [1] * (n - 2) + [0]


# ---------------------------------------------------------------- 3. malformed lanes
def test_malformed_lanes_refuse_the_batch(engine):
    S = signed(engine, 1)
    recs = records()
    pick = lambda kind: next(r for r in recs if r["kind"] == kind)
    ident = ed.SMALL_ORDER[0]
    cases = {
        "s = L": dict(pk=S.pks[40], msg=S.msgs[40], sig=S.sigs[40][:32] + le32(L)),
        "s = s + L": dict(pk=S.pks[41], msg=S.msgs[41], sig=S.sigs[41][:32] + le32(int.from_bytes(S.sigs[41][32:], "little") + L)),
        "A non-canonical": pick("A non-canonical"),                      # y = p + 1 under R = the identity, s = 0: the equation holds for the point it stands for
        "R non-canonical": pick("R non-canonical"),
        "R non-canonical, the identity": dict(pk=ident, msg=b"m", sig=le32(P + 1) + bytes(32)),
        "R off the curve": dict(pk=S.pks[42], msg=S.msgs[42], sig=le32(2) + S.sigs[42][32:]),
        "A off the curve": dict(pk=le32(2), msg=S.msgs[43], sig=S.sigs[43]),
        "A = x 0 with the sign bit": dict(pk=le32(1 | (1 << 255)), msg=b"m", sig=ident + bytes(32)),
    }
    assert ed.decode(le32(2)) is None and ed.decode(le32(P + 1)) is None
    assert both_routes(engine, Batch([ident], [b"m"], [ident + bytes(32)]), 1) == [1]         # what two of the cases are the non-canonical spelling of
    for n in (1, 17, 257):
        for name, lane in cases.items():
            assert not model.verify_cofactored(lane["pk"], lane["msg"], lane["sig"]), name
            for at in sorted({0, n - 1}):
                B = take(S, n)
                B.pks[at], B.msgs[at], B.sigs[at] = lane["pk"], lane["msg"], lane["sig"]
                assert both_routes(engine, B, 0) == [int(i != at) for i in range(n)], (name, n, at)


# ---------------------------------------------------------------- 4. mixed-order and small-order lanes
def test_mixed_order_lanes_are_accepted_whatever_their_order(engine):
    recs = records()
    mixed = [r for r in recs if r["kind"] in ed.MIXED_KINDS and not r["plain"]]
    assert len(mixed) == 224 and all(r["cof"] and r["cof_strict"] for r in mixed)
    B = batch_of(mixed)
    pk, msgs, sig, lens = B.tensors(engine)
    assert engine.ed25519_verify(pk, msgs, sig, lens=lens).cpu().tolist() == [0] * 224       # every one of them refused by the cofactorless rule
    assert both_routes(engine, B, 1) == [1] * 224
    z = device_randomizers(engine, B)
    assert z == B.model_randomizers()
    order = [int(i) for i in np.random.default_rng(4).permutation(224)]
    turned = batch_of([mixed[i] for i in order])
    assert device_randomizers(engine, turned) != [z[i] for i in order]   # other weights on the same lanes ...
    assert both_routes(engine, turned, 1) == [1] * 224                   # ... and the same verdict
    assert both_routes(engine, batch_of(mixed[::-1]), 1) == [1] * 224
    assert both_routes(engine, B, 1, small=True) == [1] * 224            # no small-order ENCODING among them: the flag changes nothing
    # with small-order lanes beside them: accepted by the equation, refused by the flag
    small = [r for r in recs if r["kind"] == "small order" and r["cof"] and not r["plain"]][:40]
    for extra in (small[:1], small, [r for r in recs if r["kind"] == "small-order A, honest R" and r["cof"]][:1]):
        if not extra:
            continue
        C2 = batch_of(mixed[:100] + list(extra) + mixed[100:])
        assert both_routes(engine, C2, 1) == [1] * len(C2)
        lanes = both_routes(engine, C2, 0, small=True)
        assert lanes == [1] * 100 + [0] * len(extra) + [1] * 124
    only_r = [r for r in recs if r["kind"] == "small order" and r["cof"] and r["pk"] == ed.SMALL_ORDER[0]][:3]
    assert only_r and both_routes(engine, batch_of(mixed[:5] + only_r), 0, small=True)[5:] == [0] * len(only_r)


def test_the_per_lane_rule_is_the_models_over_the_whole_fixture(engine):
    recs = records()
    assert len(recs) == 1019 and sum(r["cof"] and not r["plain"] for r in recs) == 676
    B = batch_of(recs)
    assert per_lane(engine, B) == [r["cof"] for r in recs]
    assert per_lane(engine, B, small=True) == [r["cof_strict"] for r in recs]
    assert per_lane(engine, B, offset=3, stride=33) == [r["cof"] for r in recs]
    assert device_randomizers(engine, B) == B.model_randomizers()        # malformed lanes included: their bytes are hashed as they are
    assert both_routes(engine, B, 0)
    good = batch_of([r for r in recs if r["cof"]])
    assert both_routes(engine, good, 1) == [1] * len(good)
    assert both_routes(engine, batch_of([r for r in recs if r["cof_strict"]]), 1, small=True)


# ---------------------------------------------------------------- 5. errors and the plan
def test_bad_arguments_are_refused_with_a_message_and_ok_is_untouched(engine):
    import torch
    from ecsimd_amd import Engine
    n = 17
    B = take(signed(engine, 112), n)
    pk, msgs, sig, _ = B.tensors(engine)
    lens = torch.full((n,), 112, dtype=torch.int32, device=engine.tdev)
    eng = Engine(0)
    try:
        lib = eng.lib
        ok = torch.full((32,), 0xAA, dtype=torch.uint8, device=eng.tdev)
        z = torch.zeros((n, 32), dtype=torch.uint8, device=eng.tdev)
        torch.cuda.synchronize()
        eng._bind_stream()
        ptr = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
        null = C.c_void_p(0)

        def batch(pkp=ptr(pk), mp=ptr(msgs), lp=null, gp=ptr(sig), okp=ptr(ok), n=n, flags=MSM, length=112, stride=112, fn="ecsimd_ed25519_verify_batch"):
            rc = getattr(lib, fn)(eng.ctx, pkp, mp, C.c_size_t(length), C.c_size_t(stride), lp, gp, okp, C.c_size_t(n), C.c_int(flags))
            return rc, lib.ecsimd_hip_last_error(eng.ctx).decode()

        def lanes(**kw):
            return batch(fn="ecsimd_ed25519_verify_cofactored", **dict(dict(flags=0), **kw))

        def randomizers(pkp=ptr(pk), mp=ptr(msgs), gp=ptr(sig), zp=ptr(z), n=n):
            rc = lib.ecsimd_ed25519_batch_randomizers(eng.ctx, pkp, mp, C.c_size_t(112), C.c_size_t(112), null, gp, zp, C.c_size_t(n))
            return rc, lib.ecsimd_hip_last_error(eng.ctx).decode()

        cases = {
            "flag 6": batch(flags=6), "flag 8": batch(flags=8), "flag -1": batch(flags=-1), "flag 16 | MSM": batch(flags=16 | MSM),
            "pk null": batch(pkp=null), "sig null": batch(gp=null), "msg null": batch(mp=null), "ok null": batch(okp=null),
            "lens misaligned": batch(lp=ptr(lens, 2)), "stride below the length": batch(stride=111),
            "ok inside pk": batch(okp=ptr(pk, 5)), "ok inside sig": batch(okp=ptr(sig, 64 * n - 1)), "ok inside msg": batch(okp=ptr(msgs, 112 * n - 1)),
            "ok inside lens": batch(lp=ptr(lens), okp=ptr(lens, 7)),
            "n too large": batch(n=(1 << 24)), "n far too large": batch(n=(1 << 40)),
            "cofactored: flag 2": lanes(flags=2), "cofactored: pk null": lanes(pkp=null), "cofactored: ok null": lanes(okp=null), "cofactored: ok is sig": lanes(okp=ptr(sig)),
            "cofactored: stride": lanes(stride=3),
            "z null": randomizers(zp=null), "z misaligned": randomizers(zp=ptr(z, 8)), "z is sig": randomizers(zp=ptr(sig)), "z inside pk": randomizers(zp=ptr(pk, 16)),
            "randomizers: n too large": randomizers(n=1 << 24), "randomizers: pk null": randomizers(pkp=null),
        }
        for name, (rc, said) in cases.items():
            assert rc == BAD_ARG and said.startswith("bad argument: ") and len(said) > 20, (name, rc, said)
        assert "overlap" in cases["ok inside sig"][1] and "overlap" in cases["z is sig"][1] and "MAX_N" in cases["n too large"][1] and "flags" in cases["flag 6"][1]
        torch.cuda.synchronize()
        assert bytes(ok.cpu().numpy()) == b"\xaa" * 32
        # a context with the reference's squaring is accepted, as in ecsimd_ed25519.h, and gives the same bytes
        eng.set_ref_square_compat(True)
        assert batch()[0] == 0 and batch(flags=LANES | SMALL, okp=ptr(ok, 1))[0] == 0 and batch(lp=ptr(lens), okp=ptr(ok, 2), flags=AUTO)[0] == 0
        assert lanes(okp=ptr(ok, 8))[0] == 0 and randomizers()[0] == 0
        eng.set_ref_square_compat(False)
        torch.cuda.synchronize()
        assert bytes(ok.cpu().numpy()) == b"\x01\x01\x01" + b"\xaa" * 5 + b"\x01" * 17 + b"\xaa" * 7
        assert [int.from_bytes(bytes(r), "little") for r in z.cpu().numpy()] == B.model_randomizers()
    finally:
        eng.close()


def test_the_plan_is_what_the_call_asks_the_workspace_for(engine):
    from ecsimd_amd import Engine
    n = 257
    B = take(signed(engine, 112), n)
    pk, msgs, sig, _ = B.tensors(engine)
    for flags in (MSM, LANES, MSM | SMALL):
        eng = Engine(0)
        try:
            plan = Engine.ed25519_batch_plan(n, 112, flags)
            assert plan["route"] == flags & ~SMALL
            levels = 3                                                   # 257 leaves: 17 nodes, 2 nodes, the root
            if plan["route"] == MSM:
                assert plan["launches"] == 5 + levels + levels + Engine.ed25519_msm_plan(n, 128)["launches"] + Engine.ed25519_msm_plan(n + 1, 253)["launches"]
            else:
                assert plan["launches"] == 3
            assert int(eng.ed25519_verify_batch(pk, msgs, sig, flags=flags).cpu()[0]) == 1
            size = C.c_size_t(0); where = C.c_void_p()
            assert eng.lib.ecsimd_hip_workspace_info(eng.ctx, C.byref(where), C.byref(size)) == 0
            assert size.value == plan["workspace_bytes"], (flags, size.value, plan)
        finally:
            eng.close()
    assert Engine.ed25519_batch_plan(n, 112, AUTO)["route"] in (MSM, LANES)


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
    n = 257
    B = take(signed(engine, 112), n)
    pk, msgs, sig, _ = B.tensors(engine)
    torch.cuda.synchronize()
    eng = Engine(0)
    try:
        oks = {route: torch.full((1,), 0xAA, dtype=torch.uint8, device=eng.tdev) for route in ROUTES}
        for route in ROUTES:                                             # the warm-up at the capture's arguments
            eng.ed25519_verify_batch(pk, msgs, sig, flags=route, out=oks[route])
        torch.cuda.synchronize()
        for route in ROUTES:
            oks[route].fill_(0xAA)
            g, _ = captured(lambda: eng.ed25519_verify_batch(pk, msgs, sig, flags=route, out=oks[route]))
            g.replay(); torch.cuda.synchronize()
            assert int(oks[route].cpu()[0]) == 1, route
            good = sig[100].clone()
            sig[100, 40] ^= 1                                            # one bit of one s overwritten in place
            torch.cuda.synchronize()
            g.replay(); torch.cuda.synchronize()
            assert int(oks[route].cpu()[0]) == 0, route
            sig[100] = good
            torch.cuda.synchronize()
            g.replay(); torch.cuda.synchronize()
            assert int(oks[route].cpu()[0]) == 1, route
            del g
    finally:
        eng.close()


def test_a_capture_without_a_warm_up_is_refused_and_stays_valid(engine):
    import torch
    from ecsimd_amd import Engine, EcsimdHipError
    n = 257
    B = take(signed(engine, 112), n)
    pk, msgs, sig, _ = B.tensors(engine)
    torch.cuda.synchronize()
    eng = Engine(0)
    try:
        ok = torch.full((1,), 0xAA, dtype=torch.uint8, device=eng.tdev)
        mark = torch.zeros((4,), dtype=torch.uint8, device=eng.tdev)
        said = {}

        def body():
            for name, fn in (("msm", lambda: eng.ed25519_verify_batch(pk, msgs, sig, flags=MSM, out=ok)), ("lanes", lambda: eng.ed25519_verify_batch(pk, msgs, sig, flags=LANES, out=ok)),
                             ("cofactored", lambda: eng.ed25519_verify_cofactored(pk, msgs, sig)), ("z", lambda: eng.ed25519_batch_randomizers(pk, msgs, sig))):
                try:
                    fn()
                except EcsimdHipError as exc:
                    said[name] = str(exc)
            mark.add_(1)                                                 # something the capture does hold
        g, _ = captured(body)
        assert sorted(said) == ["cofactored", "lanes", "msm", "z"] and all("capture" in msg and "(-1)" in msg for msg in said.values()), said
        g.replay(); torch.cuda.synchronize()
        assert int(ok.cpu()[0]) == 0xAA and mark.cpu().tolist() == [1, 1, 1, 1]
        del g
        for route in ROUTES:                                             # outside a capture the same context runs the call
            assert int(eng.ed25519_verify_batch(pk, msgs, sig, flags=route).cpu()[0]) == 1
    finally:
        eng.close()
